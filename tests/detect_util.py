"""The maximum-likelihood detection's design, shared by tests/test_detect_design.py (CPU) and tests/test_gpu_detect*.py:
the mirrors of csrc/hrt_detect.h (form rule, bit positions, LDS image), the numpy float32 emulation of the definition
in its stated order with its tie and flag rules, the case lists, the plantings, the wrong readings of the definition
that the cases separate, and the tolerance constants.

Tolerances.  Per point u = (Nr + Nt) 2^-24, a = max |S| and sigma = (|y|_2 + |H|_F a sqrt(Nt))^2; the distance of the
hard decision is compared as |d^ - d| / (u sigma) and every LLR as |llr^ - llr| N0 / (u sigma) against
hermespy_rt_amd.detect.ml_reference on the widened float32 input.  The bounds are 4 x the worst value of the float32
emulation over NORMAL_CASES, the GPU tests' own list (test_detect_design recomputes them):

    worst  metric  0.343 (n-1x1-b1)   llr  1.162 (n-1x1-b1)     bound  METRIC_BOUND = 1.372   LLR_BOUND = 4.648

The index of a point is accepted when it is the reference's, or when the reference's distance of it lies within
2 x the metric bound (times u sigma) of the reference's best; the second rule may decide at most 5 % of a case's points.
"""
import os

import numpy as np

from hermespy_rt_amd import detect as DT

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LLR = 1
NONFINITE = 1
NO_INDEX = 0xFFFFFFFF
THREADS, WAVES = 256, 4
MAX_NR, MAX_B, MAX_BITS, MAX_M, LANE_BITS = 64, 8, 12, 256, 6

METRIC_WORST, LLR_WORST = 0.343, 1.162
METRIC_BOUND, LLR_BOUND = 4 * METRIC_WORST, 4 * LLR_WORST
f32 = np.float32
FLT_MAX = np.finfo(f32).max


# ---------------------------------------------------------------- the form (csrc/hrt_detect.h)

def form(nt, b):
    """hrt_detect_form: lanes per point, min(64, Q); 0 outside the limits"""
    if not (nt >= 1 and 1 <= b <= MAX_B and nt * b <= MAX_BITS):
        return 0
    return min(64, 1 << (nt * b))


def tiles(nt, b):
    """hrt_detect_tiles: Q / g"""
    g = form(nt, b)
    return (1 << (nt * b)) // g if g else 0


def bit_position(bits, j, b):
    """hrt_detect_bit: the position in q of bit b of stream j"""
    return j * bits + (bits - 1 - b)


def lds_bytes(bits):
    """hrt_detect_lds_bytes"""
    return 8 << bits if 1 <= bits <= MAX_B else 0


def all_shapes():
    """every (Nt, B) inside the limits"""
    return [(nt, b) for b in range(1, MAX_B + 1) for nt in range(1, MAX_BITS + 1) if nt * b <= MAX_BITS]


# ---------------------------------------------------------------- the float32 emulation

def _points(H):
    """[nrx, ntx, Nr, Nt, 2, T, K] -> [nrx, ntx, 2, T, K, Nr, Nt]"""
    return np.moveaxis(np.asarray(H), (2, 3), (-2, -1))


def emulate_distances(H, Y, S, chunk=1024):
    """d_q of every point in float32, operation by operation in the definition's order: [nrx, ntx, 2, T, K, Q]"""
    H, Y, S = np.asarray(H, np.complex64), np.asarray(Y, np.complex64), np.asarray(S, np.complex64)
    nr, nt = H.shape[2], H.shape[3]
    B = S.shape[0].bit_length() - 1
    Q = 1 << (nt * B)
    Hm, Ym = _points(H), np.moveaxis(Y, 2, -1)
    hr, hi = np.ascontiguousarray(Hm.real), np.ascontiguousarray(Hm.imag)
    yr, yi = np.ascontiguousarray(Ym.real), np.ascontiguousarray(Ym.imag)
    sr, si = np.ascontiguousarray(S.real), np.ascontiguousarray(S.imag)
    d = np.empty(Hm.shape[:-2] + (Q,), f32)
    with np.errstate(all="ignore"):
        for q0 in range(0, Q, chunk):
            x = DT.hypothesis_symbols(np.arange(q0, min(Q, q0 + chunk)), nt, B)      # [c, Nt]
            dd = np.zeros(Hm.shape[:-2] + (x.shape[0],), f32)
            for i in range(nr):
                er = ei = None
                for j in range(nt):
                    a, b = hr[..., i, j, None], hi[..., i, j, None]
                    cr, ci = sr[x[:, j]], si[x[:, j]]
                    pr = a * cr - b * ci
                    pi = a * ci + b * cr
                    er = pr if j == 0 else er + pr
                    ei = pi if j == 0 else ei + pi
                rr = yr[..., i, None] - er
                ri = yi[..., i, None] - ei
                dd = dd + (rr * rr + ri * ri)
            d[..., q0:q0 + chunk] = dd
    return d


def emulate(H, Y, S, noise, llr=True):
    """The kernel in numpy float32, operation by operation: H complex64 [nrx, ntx, Nr, Nt, 2, T, K], Y complex64
    [nrx, ntx, Nr, 2, T, K], S complex64 [2^B] -> dict in the device layout: index uint32, metric float32, status uint32
    [nrx, ntx, 2, T, K], llr float32 [nrx, ntx, Nt, B, 2, T, K] (None without llr)"""
    nt = np.asarray(H).shape[3]
    B = np.asarray(S).shape[0].bit_length() - 1
    d = emulate_distances(H, Y, S)
    q = np.arange(d.shape[-1])
    n0 = f32(noise)
    with np.errstate(all="ignore"):
        bad = ~(d <= FLT_MAX).all(-1)
        safe = np.where(bad[..., None], f32(0), d)
        index = np.argmin(safe, -1)                             # the first of the smallest
        best = np.take_along_axis(safe, index[..., None], -1)[..., 0]
        L = None
        if llr:
            L = np.empty(d.shape[:-1] + (nt, B), f32)
            for j in range(nt):
                for b in range(B):
                    one = ((q >> bit_position(B, j, b)) & 1).astype(bool)
                    L[..., j, b] = (safe[..., ~one].min(-1) - safe[..., one].min(-1)) / n0
            bad = bad | ~(np.abs(L) <= FLT_MAX).all((-2, -1))
            L = np.moveaxis(np.where(bad[..., None, None], f32(0), L), (-2, -1), (2, 3)).astype(f32)
    return {"index": np.where(bad, NO_INDEX, index).astype(np.uint32), "metric": np.where(bad, f32(0), best).astype(f32),
            "status": np.where(bad, NONFINITE, 0).astype(np.uint32), "llr": L}


def rounded(ref):
    """an ml_reference result rounded to the device's types"""
    return {"index": ref["index"], "status": ref["status"], "metric": ref["metric"].astype(f32),
            "llr": None if ref["llr"] is None else ref["llr"].astype(f32)}


def same(a, b, keys=("index", "status", "metric", "llr")):
    """the first key whose arrays differ in a bit (None: all equal); -0 and +0 differ"""
    for k in keys:
        if a[k] is None or b[k] is None:
            if a[k] is not b[k]:
                return k
            continue
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return k
    return None


def out_bytes(nrx, ntx, nt, B, T, K, flags):
    """hrt_detect_out_bytes, restated"""
    pts = nrx * ntx * 2 * T * K
    return pts * 12 + (pts * nt * B * 4 if flags & LLR else 0)


# ---------------------------------------------------------------- errors against the float64 reference

def scale(H, Y, S):
    """u sigma per point [nrx, ntx, 2, T, K]: u = (Nr + Nt) 2^-24, sigma = (|y|_2 + |H|_F max|S| sqrt(Nt))^2"""
    H, Y = np.asarray(H, np.complex128), np.asarray(Y, np.complex128)
    nr, nt = H.shape[2], H.shape[3]
    a = np.abs(np.asarray(S, np.complex128)).max()
    hn = np.sqrt((np.abs(H) ** 2).sum((2, 3)))
    yn = np.sqrt((np.abs(Y) ** 2).sum(2))
    return (nr + nt) * 2.0 ** -24 * (yn + hn * a * np.sqrt(nt)) ** 2


def metric_error(metric, ref, us, index=None):
    """the worst |d^ - d| / (u sigma); with `index` (the indices that came with `metric`) only over the points where it
    is the reference's (another index accepted by the second rule is another hypothesis: not compared)"""
    e = np.abs(np.asarray(metric, np.float64) - ref["metric"]) / us
    if index is not None:
        e = np.where(np.asarray(index).astype(np.int64) == ref["index"].astype(np.int64), e, 0.0)
    return float(e.max())


def llr_error(llr, ref, us, noise):
    """the worst |llr^ - llr| N0 / (u sigma)"""
    return float((np.abs(np.asarray(llr, np.float64) - ref["llr"]) * float(noise) / us[:, :, None, None]).max())


def index_check(index, ref, us):
    """-> (every point accepted, the share accepted only by the second rule); ref holds "distances" """
    idx, rid = np.asarray(index).astype(np.int64), ref["index"].astype(np.int64)
    d = ref["distances"]
    best = d.min(-1)
    got = np.take_along_axis(d, np.where(idx == NO_INDEX, 0, idx)[..., None], -1)[..., 0]
    first = idx == rid
    second = ~first & (idx != NO_INDEX) & (got <= best + 2.0 * METRIC_BOUND * us)
    return bool((first | second).all()), float(second.mean())


def lead_share(ref, us):
    """the share of points whose float64 lead, runner-up minus best, exceeds 2 x the metric bound"""
    d = np.sort(ref["distances"], -1)
    return float((d[..., 1] - d[..., 0] > 2.0 * METRIC_BOUND * us).mean())


# ---------------------------------------------------------------- the standard-normal case list (GPU and design)

def normal(rng, shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)).astype(np.complex64)


NOISE = 0.25
# name, (nrx, ntx), Nr, Nt, B, T, K, constellation
NORMAL_CASES = (
    ("n-2x2-b2", (1, 1), 2, 2, 2, 3, 5, "qam"),
    ("n-4x4-b2", (1, 2), 4, 4, 2, 1, 7, "qam"),
    ("n-4x2-b6", (1, 1), 4, 2, 6, 1, 3, "qam"),
    ("n-4x3-b4", (1, 1), 4, 3, 4, 1, 3, "qam"),
    ("n-16x6-b2", (1, 1), 16, 6, 2, 1, 3, "qam"),
    ("n-1x1-b1", (2, 2), 1, 1, 1, 3, 3, "qam"),
    ("n-5x1-b8", (1, 1), 5, 1, 8, 1, 5, "qam"),
    ("n-7x2-b3-psk", (2, 1), 7, 2, 3, 1, 5, "psk"),
    ("n-3x5-b1", (1, 1), 3, 5, 1, 3, 3, "qam"),
)


def normal_case(case):
    """-> H complex64 [nrx, ntx, Nr, Nt, 2, T, K], Y complex64 [nrx, ntx, Nr, 2, T, K], S complex64 [2^B], the sent
    hypotheses [nrx, ntx, 2, T, K]: y = H x + noise at N0 = NOISE"""
    name, links, nr, nt, B, T, K, kind = case
    rng = np.random.default_rng(sum(name.encode()) * 7919)
    S = (DT.qam(B) if kind == "qam" else DT.psk(B, 0.1)).astype(np.complex64)
    H = normal(rng, links + (nr, nt, 2, T, K))
    sent = rng.integers(0, 1 << (nt * B), links + (2, T, K))
    X = S[DT.hypothesis_symbols(sent, nt, B)]                                   # [.., Nt]
    Y = np.einsum("...ij,...j->...i", _points(H).astype(np.complex128), X.astype(np.complex128))
    Y = np.moveaxis(Y, -1, 2) + np.sqrt(NOISE) * normal(rng, links + (nr, 2, T, K))
    return H, Y.astype(np.complex64), S, sent


def send(H, B, seed, snr=1e6):
    """-> Y complex64, S complex64, the sent hypotheses, N0: y = H x + noise of power N0 = mean |H x|^2 / snr per entry,
    the symbols from `seed`"""
    rng = np.random.default_rng(seed)
    nrx, ntx, nr, nt, _, T, K_ = H.shape
    S = DT.qam(B).astype(np.complex64)
    sent = rng.integers(0, 1 << (nt * B), (nrx, ntx, 2, T, K_))
    X = S[DT.hypothesis_symbols(sent, nt, B)].astype(np.complex128)
    Y = np.moveaxis(np.einsum("...ij,...j->...i", _points(H).astype(np.complex128), X), -1, 2)
    n0 = float(np.float32((np.abs(Y) ** 2).mean() / snr))
    Y = Y + np.sqrt(n0) * normal(rng, Y.shape)
    return Y.astype(np.complex64), S, sent, n0


# ---------------------------------------------------------------- exact plantings

def gaussian_integers(rng, shape, amp):
    return (rng.integers(-amp, amp + 1, shape) + 1j * rng.integers(-amp, amp + 1, shape)).astype(np.complex64)


# Gaussian-integer plantings: name, (nrx, ntx), Nr, Nt, B, T, K, N0.  H has entries in {-2 .. 2} (1 + j), the QAM
# coordinates are unnormalised odd integers, y = H x0 + an offset in {-1, 0, 1} (1 + j) and N0 is a power of two, so
# every d_q is an integer below 2^24 (asserted where the case is built) and every LLR is exact.  The list takes every
# (Nt, B) of the form's switches -- Q = 2, 32, 64, 128, 256, 16, 64, 64, 4096 (five ways) -- Nr = 1, 2, 5 and, at
# Q <= 64, 64, and T K = 1, 3, 4, 5, 7 and 9 points per link and polarisation, T and K odd but for T K = 4 (2 x 2):
# with 64 / Q points a wave the last wave's groups are partly empty.
INTEGER_CASES = (
    ("1x1-nr1", (1, 1), 1, 1, 1, 1, 1, 1.0),
    ("1x1-nr64", (2, 1), 64, 1, 1, 3, 1, 0.5),
    ("1x5-nr2", (1, 1), 2, 1, 5, 1, 3, 2.0),
    ("1x5-nr64", (1, 2), 64, 1, 5, 1, 5, 0.25),
    ("1x6-nr5", (1, 1), 5, 1, 6, 1, 7, 4.0),
    ("1x6-nr64", (1, 1), 64, 1, 6, 3, 1, 1.0),
    ("1x7-nr1", (2, 2), 1, 1, 7, 1, 3, 0.5),
    ("1x8-nr5", (1, 1), 5, 1, 8, 5, 1, 8.0),
    ("2x2-nr2", (1, 1), 2, 2, 2, 7, 1, 0.125),
    ("2x2-nr64", (1, 1), 64, 2, 2, 2, 2, 2.0),
    ("3x2-nr5", (1, 1), 5, 3, 2, 1, 5, 1.0),
    ("3x2-nr64", (1, 1), 64, 3, 2, 1, 1, 0.5),
    ("2x3-nr1", (1, 1), 1, 2, 3, 3, 3, 0.25),
    ("2x3-nr64", (1, 1), 64, 2, 3, 1, 3, 4.0),
    ("6x2-nr5", (1, 1), 5, 6, 2, 1, 3, 2.0),
    ("3x4-nr2", (1, 1), 2, 3, 4, 3, 1, 0.5),
    ("2x6-nr5", (1, 1), 5, 2, 6, 1, 1, 1.0),
    ("12x1-nr5", (1, 1), 5, 12, 1, 1, 3, 0.25),
    ("4x3-nr1", (1, 2), 1, 4, 3, 1, 1, 16.0),
    ("4x3-nr2", (1, 1), 2, 4, 3, 2, 2, 1.0),
)


def integer_case(case):
    """-> H, Y, S (complex64), N0, the planted hypotheses"""
    name, links, nr, nt, B, T, K, n0 = case
    rng = np.random.default_rng(sum(name.encode()) * 104729)
    S = DT.qam(B, normalised=False).astype(np.complex64)
    H = gaussian_integers(rng, links + (nr, nt, 2, T, K), 2)
    sent = rng.integers(0, 1 << (nt * B), links + (2, T, K))
    X = S[DT.hypothesis_symbols(sent, nt, B)].astype(np.complex128)
    Y = np.moveaxis(np.einsum("...ij,...j->...i", _points(H).astype(np.complex128), X), -1, 2)
    Y = Y + gaussian_integers(rng, links + (nr, 2, T, K), 1)
    return H, Y.astype(np.complex64), S, n0, sent


def _tensors(mats, ys, links, T, K):
    """H [P, Nr, Nt] and y [P, Nr] in point order -> [nrx, ntx, Nr, Nt, 2, T, K], [nrx, ntx, Nr, 2, T, K]"""
    m = np.asarray(mats).reshape(links + (2, T, K) + mats.shape[1:])
    y = np.asarray(ys).reshape(links + (2, T, K) + ys.shape[1:])
    return (np.ascontiguousarray(np.moveaxis(m, (-2, -1), (2, 3))).astype(np.complex64),
            np.ascontiguousarray(np.moveaxis(y, -1, 2)).astype(np.complex64))


def tie_cases():
    """Planted ties -> list of (name, H, Y, S, N0, the index that must win [P], the bit positions whose LLR must be +0).
    A stream whose column of H is zero does not move the distance, so all its symbols tie:
      two       Nt = 2, B = 1 (Q = 4): column 1 is zero, q and q + 2 tie; the lowest wins, LLR of stream 1 is +0
      four      Nt = 2, B = 2 (Q = 16): column 1 is zero, four hypotheses tie
      tile-edge Nt = 7, B = 1 (Q = 128): column 6 is zero, q and q | 64 tie; planted at q = 63 so that 63 and 127 = 63 | 64
                sit on both sides of the tile edge, and at q = 0 (0 and 64)"""
    out = []
    rng = np.random.default_rng(3)
    for name, nt, B, zero, sent in (("two", 2, 1, 1, (0, 1, 0, 1, 1, 0)), ("four", 2, 2, 1, (0, 3, 2, 1, 3, 2)),
                                    ("tile-edge", 7, 1, 6, (63, 0, 63, 5, 63, 0))):
        nr, P = 3, len(sent)
        S = DT.qam(B, normalised=False).astype(np.complex64)
        mats = gaussian_integers(rng, (P, nr, nt), 2)
        mats[:, 0, :] = 1 + 1j                                  # (no other column is zero)
        mats[:, :, zero] = 0
        X = S[DT.hypothesis_symbols(np.array(sent), nt, B)].astype(np.complex128)
        ys = np.einsum("pij,pj->pi", mats.astype(np.complex128), X)
        H, Y = _tensors(mats, ys, (1, 1), 1, P // 2)
        want = np.array(sent, np.uint32) & ((1 << (zero * B)) - 1)
        out.append((name, H, Y, S, 1.0, want, [bit_position(B, zero, b) for b in range(B)]))
    return out


def one_hot_case(nr, nt, B):
    """A one-hot H and y for every (row i, stream j, bit b): the point holds H[i][j] = 1 alone and y[i] = S[x] with
    x = 1 << (B - 1 - b), the label whose only set bit is b.  Stream j decides x at distance 0; the other streams'
    columns are zero, their symbols tie and the lowest (0) wins -> H, Y, S, the expected index x << (j B) [P]"""
    S = DT.qam(B, normalised=False).astype(np.complex64)
    cells = [(i, j, b) for i in range(nr) for j in range(nt) for b in range(B)]
    P = len(cells) + len(cells) % 2
    mats, ys, want = np.zeros((P, nr, nt), np.complex64), np.zeros((P, nr), np.complex64), np.zeros(P, np.uint32)
    for p in range(P):
        i, j, b = cells[p % len(cells)]
        x = 1 << (B - 1 - b)
        mats[p, i, j] = 1
        ys[p, i] = S[x]
        want[p] = x << (j * B)
    H, Y = _tensors(mats, ys, (1, 1), 1, P // 2)
    return H, Y, S, want


# ---------------------------------------------------------------- wrong readings of the definition

def reading(H, Y, S, noise, wrong):
    """ml_reference under one wrong reading of the definition (float64) -> dict as ml_reference, or None where the
    reading is not defined for the shapes"""
    H, Y, S = np.asarray(H, np.complex128), np.asarray(Y, np.complex128), np.asarray(S, np.complex128)
    nt, T = H.shape[3], H.shape[5]
    B = S.shape[0].bit_length() - 1
    if wrong == "H-conjugated":
        return DT.ml_reference(np.conj(H), Y, S, noise)
    if wrong == "H-transposed":
        return DT.ml_reference(H.swapaxes(2, 3), Y, S, noise) if H.shape[2] == nt else None
    if wrong == "constellation-conjugated":
        return DT.ml_reference(H, Y, np.conj(S), noise)
    if wrong == "digits-reversed":              # stream j takes digit Nt - 1 - j of q
        return DT.ml_reference(H[:, :, :, ::-1], Y, S, noise)
    if wrong == "noise-multiplied":
        return DT.ml_reference(H, Y, S, 1.0 / noise)
    if wrong == "Y-pol-time-swapped":           # Y's axes [2][T] read as [T][2]
        if T == 1:
            return None
        Yw = np.ascontiguousarray(Y).reshape(Y.shape[:3] + (T, 2) + Y.shape[5:]).swapaxes(3, 4)
        return DT.ml_reference(H, Yw, S, noise)
    r = DT.ml_reference(H, Y, S, noise, table=True)
    d = r.pop("distances")
    if wrong == "bits-lsb-first":
        return dict(r, llr=r["llr"][:, :, :, ::-1])
    if wrong == "llr-sign":
        return dict(r, llr=-r["llr"])
    if wrong == "minima-over-all":              # m0 = m1 = the overall minimum
        return dict(r, llr=np.zeros_like(r["llr"]))
    if wrong == "highest-on-ties":
        idx = d.shape[-1] - 1 - np.argmin(d[..., ::-1], -1)
        return dict(r, index=idx.astype(np.uint32))
    if wrong == "unsquared":                    # sum_i |r_i| for sum_i |r_i|^2
        Hm, Ym = _points(H), np.moveaxis(Y, 2, -1)
        q = np.arange(d.shape[-1])
        X = S[DT.hypothesis_symbols(q, nt, B)]
        du = np.abs(Ym[..., None, :] - np.einsum("...ij,cj->...ci", Hm, X)).sum(-1)
        L = np.empty(du.shape[:-1] + (nt, B))
        for j in range(nt):
            for b in range(B):
                one = ((q >> bit_position(B, j, b)) & 1).astype(bool)
                L[..., j, b] = (du[..., ~one].min(-1) - du[..., one].min(-1)) / noise
        return dict(r, index=np.argmin(du, -1).astype(np.uint32), metric=du.min(-1),
                    llr=np.moveaxis(L, (-2, -1), (2, 3)))
    if wrong == "out-pol-time-swapped":         # the outputs' axes [2][T] laid out as [T][2]
        if T == 1:
            return None
        return {k: np.ascontiguousarray(v).reshape(v.shape[:-3] + (T, 2) + v.shape[-1:]).swapaxes(-3, -2)
                for k, v in r.items()}
    if wrong == "llr-streams-reversed":         # LLRs of stream j written at stream Nt - 1 - j
        return dict(r, llr=r["llr"][:, :, ::-1])
    raise ValueError(wrong)


WRONG_READINGS = ("H-conjugated", "H-transposed", "constellation-conjugated", "digits-reversed", "bits-lsb-first",
                  "llr-sign", "noise-multiplied", "minima-over-all", "highest-on-ties", "unsquared",
                  "Y-pol-time-swapped", "out-pol-time-swapped", "llr-streams-reversed")
