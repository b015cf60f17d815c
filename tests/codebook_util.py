"""The codebook selection's design, shared by tests/test_codebook_design.py (CPU) and tests/test_gpu_codebook*.py: the
mirrors of csrc/hrt_codebook.h (tile rule, LDS image, log2 restatement), the numpy float32 emulation of the kernel's
sums in the kernel's order, the case lists, the wrong readings of the definition that the cases separate, and the
tolerance constants.

Tolerances.  With u = (Nr + Nt) 2^-24 the score of every entry is compared as |mu^ - mu| / (u (1 + |mu|)) against
hermespy_rt_amd.codebook.select_reference on the widened float32 input, and the effective channel as
|E^ - E|_F / (u |H|_F |W|_F) per point (W the selected entry).  The bounds are 4 x the worst value of the float32
emulation over NORMAL_CASES, the GPU tests' own list, both metrics (test_codebook_design recomputes them):

    worst  mu  0.411 (dp1-3x4, power)   effective  0.382 (rnd1-1x2)     bound  MU_BOUND = 1.644   EFF_BOUND = 1.528

The index of a subband is accepted when it is the reference's, or when the reference's score of it is within
2 x the score bound of the reference's best; the second rule may decide at most 5 % of a case's subbands.
"""
import os

import numpy as np

from hermespy_rt_amd import codebook as CB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

POWER, CAPACITY = 0, 1
TABLE, EFFECTIVE = 1, 2
NONFINITE = 1
NO_INDEX = 0xFFFFFFFF
METRIC_NAME = {POWER: "power", CAPACITY: "capacity"}
THREADS, WAVES, LDS_BYTES = 256, 4, 65536
MAX_NR, MAX_NT, MAX_L, MAX_C, ROWS = 16, 64, 4, 4096, 4
SQRT2_BITS = 0x3FB504F3
LOG2_C = tuple(np.float32(2.0 / ((2 * j + 1) * np.log(2.0))) for j in range(5))

MU_WORST, EFF_WORST = 0.411, 0.382
MU_BOUND, EFF_BOUND = 4 * MU_WORST, 4 * EFF_WORST
f32 = np.float32


# ---------------------------------------------------------------- the form (csrc/hrt_codebook.h)

def tile(nt, l):
    """hrt_codebook_tile"""
    if not (1 <= nt <= MAX_NT and 1 <= l <= MAX_L and l <= nt):
        return 0
    return 64 if 64 * nt * l * 8 <= LDS_BYTES else 32


def slot(ct, L, j, t, l):
    """hrt_codebook_slot: the float2 slot of element (t, l) of the tile's entry j"""
    return (t * L + l) * ct + j


def banks_b64(slots):
    """the worst number of distinct addresses that meet in one LDS bank when a wave reads or writes one float2 per lane
    at these float2 slots: 64 banks of 4 bytes, a 64-bit access is served in two halves of 32 lanes"""
    worst = 1
    s = np.asarray(slots, np.int64)
    for half in (s[:32], s[32:]):
        if half.size:
            words = np.unique(np.concatenate([2 * half, 2 * half + 1]))
            worst = max(worst, int(np.bincount(words % 64).max()))
    return worst


# ---------------------------------------------------------------- the log2 restatement

def log2_f32(x):
    """hrt_cs_log2 on a float32 array, operation by operation"""
    x = np.asarray(x, f32)
    u = x.view(np.uint32)
    ok = (u >= 0x00800000) & (u < 0x7F800000)
    u = np.where(ok, u, np.uint32(0x3F800000))
    e = (u >> 23).astype(np.int32) - 127
    m = (u & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)
    big = m > SQRT2_BITS
    m = np.where(big, m - np.uint32(0x00800000), m).astype(np.uint32)
    e = e + big
    f = m.view(f32)
    s = (f - f32(1)) / (f + f32(1))
    z = s * s
    p = LOG2_C[3] + z * LOG2_C[4]
    p = LOG2_C[2] + z * p
    p = LOG2_C[1] + z * p
    p = LOG2_C[0] + z * p
    r = e.astype(f32) + s * p
    return np.where(ok, r, f32(np.nan)).astype(f32)


# ---------------------------------------------------------------- the float32 emulation

def _points(H):
    """[nrx, ntx, Nr, Nt, 2, T, K] -> [nrx, ntx, 2, T, K, Nr, Nt]"""
    return np.moveaxis(np.asarray(H), (2, 3), (-2, -1))


def _rows(hr, hi, wr, wi):
    """er, ei [.., Nr, L] = sum over t ascending of h[.., Nr, t] w[.., t, L], the kernel's statement (h broadcast
    against w over the leading axes)"""
    nt = hr.shape[-1]
    er = ei = f32(0)
    for t in range(nt):
        xr, xi = hr[..., :, t, None], hi[..., :, t, None]
        yr, yi = wr[..., None, t, :], wi[..., None, t, :]
        er = er + (xr * yr - xi * yi)
        ei = ei + (xr * yi + xi * yr)
    return er, ei


def _value(er, ei, metric, n0):
    """f(E) of [.., Nr, L] -> [..], the kernel's statements"""
    nr, L = er.shape[-2:]
    gd = [f32(0)] * L
    gr = [[f32(0)] * L for _ in range(L)]
    gi = [[f32(0)] * L for _ in range(L)]
    for i in range(nr):
        for a in range(L):
            ra, ia = er[..., i, a], ei[..., i, a]
            gd[a] = gd[a] + (ra * ra + ia * ia)
            if metric == CAPACITY:
                for b in range(a):
                    rb, ib = er[..., i, b], ei[..., i, b]
                    gr[a][b] = gr[a][b] + (ra * rb + ia * ib)
                    gi[a][b] = gi[a][b] + (ra * ib - ia * rb)
    if metric == POWER:
        f = gd[0]
        for a in range(1, L):
            f = f + gd[a]
        return f
    n0 = f32(n0)
    det = None
    for j in range(L):
        for m in range(j):
            vr, vi = gr[j][m] / n0, gi[j][m] / n0
            for p in range(m):
                vr = vr - (gr[j][p] * gr[m][p] + gi[j][p] * gi[m][p]) * gd[p]
                vi = vi - (gi[j][p] * gr[m][p] - gr[j][p] * gi[m][p]) * gd[p]
            gr[j][m] = vr / gd[m]
            gi[j][m] = vi / gd[m]
        d = f32(1) + gd[j] / n0
        for m in range(j):
            d = d - (gr[j][m] * gr[j][m] + gi[j][m] * gi[j][m]) * gd[m]
        gd[j] = d
        det = d if j == 0 else det * d
    return log2_f32(det)


def emulate(H, W, metric, noise=None, subband=None, chunk=64):
    """The kernel in numpy float32, operation by operation: H complex64 [nrx, ntx, Nr, Nt, 2, T, K], W complex64
    [C, Nt, L] -> dict in the device layout: index uint32, metric float32, status uint32 [nrx, ntx, 2, T, B], table
    float32 [nrx, ntx, C, 2, T, B], effective complex64 [nrx, ntx, Nr, L, 2, T, K]"""
    H, W = np.asarray(H, np.complex64), np.asarray(W, np.complex64)
    nrx, ntx, nr, nt, _, T, K = H.shape
    Cn, _, L = W.shape
    S, B, bands = CB.subbands(K, subband)
    Hm = _points(H)
    hr, hi = np.ascontiguousarray(Hm.real), np.ascontiguousarray(Hm.imag)        # [.., K, Nr, Nt]
    wr, wi = np.ascontiguousarray(W.real), np.ascontiguousarray(W.imag)
    table = np.empty((nrx, ntx, 2, T, B, Cn), f32)
    with np.errstate(all="ignore"):
        for c0 in range(0, Cn, chunk):
            er, ei = _rows(hr[..., None, :, :], hi[..., None, :, :], wr[c0:c0 + chunk], wi[c0:c0 + chunk])
            f = _value(er, ei, metric, noise)                                    # [.., K, c]
            for b, (k0, n) in enumerate(bands):
                s = f[..., k0, :]
                for kk in range(1, n):
                    s = s + f[..., k0 + kk, :]
                table[..., b, c0:c0 + chunk] = s / f32(n)
        bad = ~(np.abs(table) <= np.finfo(f32).max).all(-1)
        index = np.argmax(np.where(bad[..., None], f32(0), table), axis=-1)      # the first of the largest
        best = np.take_along_axis(table, index[..., None], -1)[..., 0]
        eff = np.zeros((nrx, ntx, 2, T, K, nr, L), np.complex64)
        for b, (k0, n) in enumerate(bands):
            sel = index[..., b]
            er, ei = _rows(hr[..., k0:k0 + n, :, :], hi[..., k0:k0 + n, :, :], wr[sel][..., None, :, :],
                           wi[sel][..., None, :, :])
            E = (er + 1j * ei).astype(np.complex64)
            eff[..., k0:k0 + n, :, :] = np.where(bad[..., b][..., None, None, None], 0, E)
    table = np.where(bad[..., None], f32(0), table)
    return {"index": np.where(bad, NO_INDEX, index).astype(np.uint32), "metric": np.where(bad, f32(0), best).astype(f32),
            "status": np.where(bad, NONFINITE, 0).astype(np.uint32), "table": np.moveaxis(table, -1, 2),
            "effective": np.moveaxis(eff, (-2, -1), (2, 3))}


def rounded(ref):
    """a select_reference result rounded to the device's types"""
    return {"index": ref["index"], "status": ref["status"], "metric": ref["metric"].astype(f32),
            "table": ref["table"].astype(f32), "effective": ref["effective"].astype(np.complex64)}


def same(a, b, keys=("index", "status", "metric", "table", "effective")):
    """the first key whose arrays differ in a bit (None: all equal); -0 and +0 differ"""
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return k
    return None


def out_bytes(nrx, ntx, nr, T, K, L, Cn, S, flags):
    """hrt_codebook_out_bytes, restated"""
    B = (K + S - 1) // S
    sub = nrx * ntx * 2 * T * B
    return sub * 12 + (sub * Cn * 4 if flags & TABLE else 0) + (nrx * ntx * 2 * T * K * nr * L * 8 if flags & EFFECTIVE else 0)


# ---------------------------------------------------------------- errors against the float64 reference

def mu_error(table, ref_table, nr, nt):
    """the worst |mu^ - mu| / (u (1 + |mu|))"""
    u = (nr + nt) * 2.0 ** -24
    t, r = np.asarray(table, np.float64), np.asarray(ref_table, np.float64)
    return float((np.abs(t - r) / (u * (1.0 + np.abs(r)))).max())


def eff_error(eff, ref, H, W, index=None):
    """the worst |E^ - E|_F / (u |H|_F |W_c*|_F) over the points, W_c* the reference's selected entry; with `index`
    (the indices that came with eff) only over the subbands where it is the reference's"""
    nrx, ntx, nr, nt, _, T, K = H.shape
    u = (nr + nt) * 2.0 ** -24
    S = (K + ref["index"].shape[-1] - 1) // ref["index"].shape[-1]
    d = np.sqrt((np.abs(np.asarray(eff, np.complex128) - ref["effective"]) ** 2).sum((2, 3)))      # [nrx, ntx, 2, T, K]
    hn = np.sqrt((np.abs(np.asarray(H, np.complex128)) ** 2).sum((2, 3)))
    wn = np.sqrt((np.abs(np.asarray(W, np.complex128)) ** 2).sum((1, 2)))
    idx = np.repeat(ref["index"].astype(np.int64), S, axis=-1)[..., :K]
    den = u * hn * wn[np.where(idx == NO_INDEX, 0, idx)]
    e = d / np.where(den > 0, den, 1.0)
    if index is not None:           # (another index accepted by the second rule is another entry: not compared)
        e = np.where(np.repeat(np.asarray(index).astype(np.int64), S, axis=-1)[..., :K] == idx, e, 0.0)
    return float(e.max())


def index_check(index, ref, nr, nt):
    """-> (every subband accepted, the share accepted only by the second rule): a device index is accepted when it is
    the reference's, or when the reference's score of it is within 2 x the score bound of the reference's best"""
    idx, rid = np.asarray(index).astype(np.int64), ref["index"].astype(np.int64)
    tab = np.moveaxis(ref["table"], 2, -1)
    best = tab.max(-1)
    got = np.take_along_axis(tab, np.where(idx == NO_INDEX, 0, idx)[..., None], -1)[..., 0]
    tol = 2.0 * MU_BOUND * (nr + nt) * 2.0 ** -24 * (1.0 + np.abs(best))
    first = idx == rid
    second = ~first & (idx != NO_INDEX) & (got >= best - tol)
    return bool((first | second).all()), float(second.mean())


def lead_share(ref, nr, nt):
    """the share of subbands whose float64 lead, best minus runner-up, exceeds 2 x the score bound (1 for C = 1)"""
    tab = np.sort(np.moveaxis(ref["table"], 2, -1), -1)
    if tab.shape[-1] < 2:
        return 1.0
    tol = 2.0 * MU_BOUND * (nr + nt) * 2.0 ** -24 * (1.0 + np.abs(tab[..., -1]))
    return float((tab[..., -1] - tab[..., -2] > tol).mean())


# ---------------------------------------------------------------- the standard-normal case list (GPU and design)

def normal(rng, shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)).astype(np.complex64)


def random_codebook(rng, Cn, nt, L):
    """entries of unit Frobenius norm"""
    W = rng.standard_normal((Cn, nt, L)) + 1j * rng.standard_normal((Cn, nt, L))
    return (W / np.sqrt((np.abs(W) ** 2).sum((1, 2), keepdims=True))).astype(np.complex64)


NOISE = 0.25
# name, (nrx, ntx), Nr, Nt, T, K, S, codebook.  The dual-polarised codebooks are the rank-1 ones: the two co-phases of a
# rank-2 entry [[v, v]; [phi v, -phi v]] give the same |E|_F^2 and the same det(I + E^H E / N0) for every H (E is
# [H1 v, phi H2 v] times a scaled unitary matrix), so they tie mathematically and no lead separates them; Nt = 1 ties
# likewise under unit-norm entries.  Those shapes are pinned by the exact plantings instead.
NORMAL_CASES = (
    ("dp1-2x8", (1, 1), 2, 8, 1, 24, 12, ("dual", 4, 4, 1)),
    ("dp1-4x32", (1, 2), 4, 32, 1, 14, 12, ("dual", 16, 4, 1)),
    ("dp1-3x4", (2, 2), 3, 4, 3, 5, 2, ("dual", 2, 2, 1)),
    ("rnd1-1x2", (1, 1), 1, 2, 1, 9, 4, ("random", 3, 1)),
    ("rnd1-1x33", (1, 1), 1, 33, 1, 6, 6, ("random", 65, 1)),
    ("rnd3-5x33", (1, 1), 5, 33, 1, 5, 4, ("random", 65, 3)),
    ("rnd3-16x63", (1, 1), 16, 63, 1, 3, 2, ("random", 33, 3)),
    ("rnd4-16x64", (1, 1), 16, 64, 1, 4, 3, ("random", 65, 4)),
    ("rnd4-4x4", (1, 1), 4, 4, 2, 8, 8, ("random", 129, 4)),
)


def normal_case(case):
    """-> H complex64 [nrx, ntx, Nr, Nt, 2, T, K], W complex64 [C, Nt, L], S"""
    name, links, nr, nt, T, K, S, cb = case
    rng = np.random.default_rng(sum(name.encode()) * 7919)
    H = normal(rng, links + (nr, nt, 2, T, K))
    if cb[0] == "dual":
        W = CB.dual_polarised(cb[1], cb[2], cb[3]).astype(np.complex64)
    else:
        W = random_codebook(rng, cb[1], nt, cb[2])
    assert W.shape[1] == nt
    return H, W, S


# ---------------------------------------------------------------- exact plantings

def _tensor(mats, links, T, K):
    """[links[0] links[1] 2 T K, Nr, Nt] in point order -> [nrx, ntx, Nr, Nt, 2, T, K]"""
    m = np.asarray(mats).reshape(links + (2, T, K) + mats.shape[1:])
    return np.ascontiguousarray(np.moveaxis(m, (-2, -1), (2, 3)))


def gaussian_integers(rng, shape, amp, fill=1.0):
    z = rng.integers(-amp, amp + 1, shape) + 1j * rng.integers(-amp, amp + 1, shape)
    return (z * (rng.random(shape) < fill)).astype(np.complex64)


# Gaussian-integer plantings under POWER: name, links, Nr, Nt, L, C, T, K, S, amplitude, fill.  The list covers every
# value of every axis of the issue's list and the tile edges of both tile sizes (CT 64: 63, 64, 65, 129; CT 32, taken
# at Nt L > 128: 31, 32, 33, 65); S is a power of two and K leaves a last subband of 1 or S frequencies, so every
# mean is exact; every sum stays below 2^24 (asserted where the case is built).
INTEGER_CASES = (
    ("1x1-c1", (1, 1), 1, 1, 1, 1, 1, 1, 1, 3, 1.0),
    ("1x4-c2", (1, 1), 1, 4, 1, 2, 1, 5, 1, 3, 1.0),
    ("2x4-l2-c63", (1, 1), 2, 4, 2, 63, 3, 5, 2, 3, 1.0),
    ("2x4-l3-c64", (1, 1), 2, 4, 3, 64, 1, 5, 4, 3, 1.0),
    ("3x4-l4-c65", (2, 2), 3, 4, 4, 65, 1, 5, 4, 3, 1.0),
    ("3x33-l1-c129", (1, 1), 3, 33, 1, 129, 1, 5, 2, 2, 1.0),
    ("2x4-l1-c1023", (1, 1), 2, 4, 1, 1023, 1, 5, 4, 3, 1.0),
    ("1x4-l2-c1024", (1, 1), 1, 4, 2, 1024, 1, 1, 1, 3, 1.0),
    ("2x4-l1-c1025", (1, 1), 2, 4, 1, 1025, 1, 5, 4, 3, 1.0),
    ("16x63-l3-c31", (1, 1), 16, 63, 3, 31, 1, 5, 4, 1, 0.5),
    ("16x64-l4-c32", (1, 1), 16, 64, 4, 32, 1, 1, 1, 1, 0.5),
    ("3x64-l3-c33", (1, 1), 3, 64, 3, 33, 1, 5, 4, 1, 0.5),
    ("2x64-l4-c65", (1, 1), 2, 64, 4, 65, 3, 1, 1, 1, 0.5),
    ("16x33-l2-k64", (1, 1), 16, 33, 2, 5, 1, 64, 64, 1, 0.25),
    ("3x33-l4-k64", (1, 1), 3, 33, 4, 64, 1, 64, 2, 1, 0.5),
    ("1x63-l1-k64-s1", (1, 1), 1, 63, 1, 65, 1, 64, 1, 1, 1.0),
)


def integer_case(case):
    name, links, nr, nt, L, Cn, T, K, S, amp, fill = case
    rng = np.random.default_rng(sum(name.encode()) * 104729)
    H = gaussian_integers(rng, links + (nr, nt, 2, T, K), amp, fill)
    W = gaussian_integers(rng, (Cn, nt, L), amp, fill)
    return H, W, S


def capacity_l1_case(nr=3, nt=5, K=8, S=4, links=(1, 2), T=1):
    """L = 1 under CAPACITY with 1 + |E|^2 / N0 a power of two: one-hot entries pick a column of H, and the columns'
    squared norms are 0, 1, 3, 7 or 15 (four squares, spread over two rows), N0 = 1 -> H, W, S, N0.  Entries beyond
    Nt repeat earlier ones (ties)."""
    rng = np.random.default_rng(77)
    four = {0: (0, 0, 0, 0), 1: (1, 0, 0, 0), 3: (1, 1, 1, 0), 7: (2, 1, 1, 1), 15: (3, 2, 1, 1)}
    pts = links[0] * links[1] * 2 * T * K
    mats = np.zeros((pts, nr, nt), np.complex64)
    for p in range(pts):
        for t in range(nt):
            a, b, c, d = four[int(rng.choice(list(four)))]
            i, j = rng.choice(nr, 2, replace=False)
            mats[p, i, t] = a + 1j * b
            mats[p, j, t] = c + 1j * d
    W = np.zeros((nt + 3, nt, 1), np.complex64)
    for c in range(nt + 3):
        W[c, c % nt, 0] = 1
    return _tensor(mats, links, T, K), W, S, 1.0


def one_hot_case(nr, nt, L):
    """One-hot H and one-hot entries for every (row, column, layer, entry): point p = i nt + t holds H[i][t] = 1, entry
    c = t L + l holds W[t][l] = l + 1, so under POWER the point (i, t) selects c = t L + L - 1 with metric L^2 and its
    effective channel is L at (i, L - 1) -> H [1, 1, Nr, Nt, 2, 1, K], W, expected index per point [2 K]"""
    pts = nr * nt
    K = (pts + 1) // 2
    mats = np.zeros((2 * K, nr, nt), np.complex64)
    want = np.zeros(2 * K, np.uint32)
    for p in range(2 * K):
        i, t = (p % pts) // nt, (p % pts) % nt
        mats[p, i, t] = 1
        want[p] = t * L + L - 1
    W = np.zeros((nt * L, nt, L), np.complex64)
    for t in range(nt):
        for l in range(L):
            W[t * L + l, t, l] = l + 1
    return _tensor(mats, (1, 1), 1, K), W, want


def tie_case():
    """planted ties: entries c and c' > c equal, both the best -> H, W, S, the index that must win"""
    rng = np.random.default_rng(5)
    H = gaussian_integers(rng, (1, 1, 2, 4, 2, 1, 4), 2)
    W = gaussian_integers(rng, (70, 4, 2), 1)
    W[3] = W[66] = 3 * np.array([[1, 1j], [1, 0], [0, 1], [1j, 1]])
    W[66 + 1] = W[3]
    return H, W, 2, 3


# ---------------------------------------------------------------- wrong readings of the definition

def reading(H, W, metric, noise, subband, wrong):
    """select_reference under one wrong reading of the definition (float64) -> dict as select_reference, or None where
    the reading is not defined for the shapes"""
    H, W = np.asarray(H, np.complex128), np.asarray(W, np.complex128)
    K = H.shape[6]
    S = K if subband is None else subband
    if wrong == "conjugated":
        return CB.select_reference(H, np.conj(W), metric, noise, S)
    if wrong == "transposed":                   # W_c^T where it is square; otherwise not defined
        return CB.select_reference(H, np.swapaxes(W, 1, 2), metric, noise, S) if W.shape[1] == W.shape[2] else None
    if wrong == "layout":                       # [C][L][Nt] read as [C][Nt][L]
        return CB.select_reference(H, np.ascontiguousarray(W.swapaxes(1, 2)).reshape(W.shape), metric, noise, S)
    if wrong == "power-under-capacity":
        return CB.select_reference(H, W, POWER, noise, S)
    if wrong == "noise-multiplied":
        return CB.select_reference(H, W, metric, 1.0 / noise, S)
    if wrong == "pol-time-swapped":
        # the outputs' axes [2][T] laid out, or viewed, as [T][2] while H is read as it is ((pol, T) are the axes -3, -2
        # of every region; the kernel itself only ever uses pol T + m, so a swap on both sides would be no error)
        T = H.shape[5]
        if T == 1:
            return None
        r = CB.select_reference(H, W, metric, noise, S)
        return {k: np.ascontiguousarray(v).reshape(v.shape[:-3] + (T, 2) + v.shape[-1:]).swapaxes(-3, -2)
                for k, v in r.items()}
    r = CB.select_reference(H, W, metric, noise, S)
    B = r["index"].shape[-1]
    n = np.array([min(S, K - b * S) for b in range(B)], np.float64)
    if wrong == "sum":
        return dict(r, metric=r["metric"] * n, table=r["table"] * n)
    if wrong == "last-by-S":
        return dict(r, metric=r["metric"] * n / S, table=r["table"] * n / S)
    if wrong == "highest-on-ties":
        tab = np.moveaxis(r["table"], 2, -1)
        idx = tab.shape[-1] - 1 - np.argmax(tab[..., ::-1], -1)
        return dict(r, index=idx.astype(np.uint32))
    if wrong == "trace":                        # log2(1 + tr G / N0) for log2 det
        Hm = _points(H)
        tab = np.empty_like(r["table"])
        for c in range(W.shape[0]):
            f = np.log2(1.0 + (np.abs(Hm @ W[c]) ** 2).sum((-2, -1)) / noise)
            for b in range(B):
                tab[:, :, c, :, :, b] = f[..., b * S:b * S + int(n[b])].sum(-1) / n[b]
        return dict(r, table=tab, metric=tab.max(2), index=np.argmax(tab, 2).astype(np.uint32))
    if wrong == "neighbour-effective":          # effective from c* of the neighbouring subband
        if B < 2:
            return None
        Hm = _points(H)
        eff = np.moveaxis(r["effective"], (2, 3), (-2, -1)).copy()
        for b in range(B):
            sel = r["index"][..., (b + 1) % B].astype(np.int64)
            k0 = b * S
            eff[..., k0:k0 + int(n[b]), :, :] = Hm[..., k0:k0 + int(n[b]), :, :] @ W[sel][..., None, :, :]
        return dict(r, effective=np.moveaxis(eff, (-2, -1), (2, 3)))
    raise ValueError(wrong)


WRONG_READINGS = ("conjugated", "transposed", "layout", "sum", "last-by-S", "highest-on-ties", "noise-multiplied",
                  "trace", "pol-time-swapped", "neighbour-effective", "power-under-capacity")
