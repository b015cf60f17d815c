"""Planted cases of the received-signal family (hrt_propagate, Tracer.apply_taps), no GPU needed to build them:
the exact (integer) planting and its covering set of shapes, the one-hot pairs, a Python mirror of the form rule of
csrc/hrt_propagate.h, and an evaluator of the definition with switches for eight wrong readings of it (the mutants the
planted cases must catch; tests/test_propagate_design.py)."""
import numpy as np

from hermespy_rt_amd import propagate as pg

# ---------------------------------------------------------------------------------------------- the form rule

MFMA, GENERAL = "mfma", "general"
COLS, LC, WTILES = 256, 256, 4   # csrc/hrt_propagate.h: HRT_PG_COLS, HRT_PG_LC, HRT_PG_WTILES


def form(num_times, samples_per_block):
    """mirror of hrt_propagate_form: MFMA where a 16-column tile cannot straddle two blocks"""
    return MFMA if num_times == 1 or samples_per_block % 16 == 0 else GENERAL


def b_read_banks(nl, lc, d0):
    """the LDS banks (ds_read_b32: dword mod 32) the 64 lanes of a wave read for the B operand of one k step: lane =
    16 kq + col reads dword 2 (nl + col + lc - (d0 + (kq >> 1))) + (kq & 1) of the interleaved window"""
    lanes = np.arange(64)
    kq, col = lanes >> 4, lanes & 15
    return (2 * (nl + col + lc - (d0 + (kq >> 1))) + (kq & 1)) % 32


# ---------------------------------------------------------------------------------------------- the definition

MUTANTS = ("no_clamp", "m_from_input", "lmin_sign", "conj_h", "swap_pol_element", "tx0_only", "wrap_x", "cut_tail")


def evaluate(h, x, l_min, S, n_out, mutant=None):
    """The definition, tap by tap over all samples at once (complex128; exact on small integers) -> [nrx, Nr, 2,
    n_out].  S None: one block.  `mutant`: one of MUTANTS, a wrong reading of the definition."""
    assert mutant is None or mutant in MUTANTS
    h = np.asarray(h, np.complex128)
    x = np.asarray(x, np.complex128)
    nrx, ntx, nr, nt, _, M, L = h.shape
    N = x.shape[2]
    S = max(n_out, 1) if S is None else S
    if mutant == "conj_h":
        h = h.conj()
    if mutant == "lmin_sign":
        l_min = -l_min
    n = np.arange(n_out)
    y = np.zeros((nrx, nr, 2, n_out), np.complex128)
    for l in range(L):
        k = n - l_min - l
        if mutant == "wrap_x":
            ok, kk = np.ones(n_out, bool), k % N
        else:
            ok, kk = (k >= 0) & (k < N), np.clip(k, 0, N - 1)
        m = (np.clip(k, 0, None) if mutant == "m_from_input" else n) // S
        if mutant == "no_clamp":
            ok = ok & (m < M)
        m = np.minimum(m, M - 1)
        hl = h[:, :, :, :, :, m, l]                      # [nrx, ntx, nr, nt, 2, n]
        xl = np.where(ok, x[:, :, kk], 0)                # [ntx, nt, n]
        if mutant == "tx0_only":
            hl, xl = hl[:, :1], xl[:1]
        y += np.einsum("rtijpn,tjn->ripn", hl, xl)
    if mutant == "cut_tail":
        y[..., N:] = 0
    if mutant == "swap_pol_element":   # rows laid out [pol][i], read back as [i][pol]
        y = np.ascontiguousarray(y.transpose(0, 2, 1, 3)).reshape(nrx, nr, 2, n_out)
    return y


def convolve_reference(h, x, l_min, S, n_out):
    """an independent formulation: np.convolve of every (row, port) per block, the blocks stitched together"""
    h = np.asarray(h, np.complex128)
    x = np.asarray(x, np.complex128)
    nrx, ntx, nr, nt, _, M, L = h.shape
    N = x.shape[2]
    S = max(n_out, 1) if S is None else S
    y = np.zeros((nrx, nr, 2, n_out), np.complex128)
    for m in range(M):
        lo, hi = m * S, (n_out if m == M - 1 else min((m + 1) * S, n_out))
        if lo >= hi:
            continue
        for rx in range(nrx):
            for i in range(nr):
                for pol in range(2):
                    full = np.zeros(N + L - 1, np.complex128)
                    for tx in range(ntx):
                        for j in range(nt):
                            full += np.convolve(h[rx, tx, i, j, pol, m], x[tx, j])
                    for nn in range(lo, hi):   # y[n] = full[n - l_min]
                        q = nn - l_min
                        if 0 <= q < N + L - 1:
                            y[rx, i, pol, nn] = full[q]
    return y


# ---------------------------------------------------------------------------------------------- the exact planting

AXES = {
    "L": (1, 2, 3, 4, 5, 16, 17),
    "rows": ((1, 1), (1, 3), (1, 4), (1, 5), (3, 3)),          # (nrx, Nr): 2, 6, 8, 10, 18 complex rows
    "ports": ((1, 1), (2, 1), (1, 3), (2, 3)),                 # (ntx, Nt)
    "N": (1, 15, 16, 17, 40),
    "n_out": ("N-3", "N", "N+L-1", "N+L+20"),
    "l_min": (0, -3, 5, "-(N+L)", "N+40"),
    # (S, M): MFMA form, general form (M "n_out": per-sample), and the time-invariant channel (S None)
    "blocks": ((16, 1), (16, 3), (32, 2), (48, 1), (1, "n_out"), (5, 4), (17, 2), (None, 1)),
}


def _resolve(c):
    """a choice of one value per axis -> the concrete case"""
    L, N = c["L"], c["N"]
    n_out = max({"N-3": N - 3, "N": N, "N+L-1": N + L - 1, "N+L+20": N + L + 20}[c["n_out"]], 1)
    l_min = {"-(N+L)": -(N + L), "N+40": N + 40}.get(c["l_min"], c["l_min"])
    S, M = c["blocks"]
    M = n_out if M == "n_out" else M
    return dict(nrx=c["rows"][0], nr=c["rows"][1], ntx=c["ports"][0], nt=c["ports"][1], L=L, N=N, n_out=n_out,
                l_min=l_min, S=S, M=M, choice=dict(c))


def covered(choices):
    """every value of every axis appears with at least two values of every other axis"""
    for a, values in AXES.items():
        for v in values:
            mine = [c for c in choices if c[a] == v]
            for b in AXES:
                if b != a and len({c[b] for c in mine}) < 2:
                    return False
    return True


def exact_cases():
    """a covering subset of the cross product of AXES (deterministic): random choices until `covered` holds"""
    rng = np.random.RandomState(20240)
    names = sorted(AXES)
    choices = []
    while not covered(choices):
        choices.append({a: AXES[a][rng.randint(len(AXES[a]))] for a in names})
        assert len(choices) < 400
    return [_resolve(c) for c in choices]


def plant_integers(case, seed=0):
    """h [nrx, ntx, Nr, Nt, 2, M, L] and x [ntx, Nt, N] complex64 with Re, Im drawn from {-2 .. 2}: every partial sum
    is an integer below 2^24, exact in float32 in any order"""
    rng = np.random.RandomState(seed)
    hs = (case["nrx"], case["ntx"], case["nr"], case["nt"], 2, case["M"], case["L"])
    xs = (case["ntx"], case["nt"], case["N"])
    h = rng.randint(-2, 3, hs) + 1j * rng.randint(-2, 3, hs)
    x = rng.randint(-2, 3, xs) + 1j * rng.randint(-2, 3, xs)
    assert 8 * case["ntx"] * case["nt"] * case["L"] < 1 << 24
    return h.astype(np.complex64), x.astype(np.complex64)


def reference(case, h, x):
    return pg.apply_taps_reference(h, x, case["l_min"], case["S"], case["n_out"])


# ---------------------------------------------------------------------------------------------- one-hot pairs

ONE_HOT_SHAPE = dict(nrx=2, ntx=2, nr=3, nt=2, M=3, L=5, N=40, n_out=64)
ONE_HOT_AXES = ("rx", "tx", "i", "j", "pol", "m", "l", "n0")


def one_hot_cases():
    """(S, index dict) pairs: both forms; all axes at their first index, all at their last, and each axis alone moved
    to the other end from either base"""
    s = ONE_HOT_SHAPE
    last = dict(rx=s["nrx"] - 1, tx=s["ntx"] - 1, i=s["nr"] - 1, j=s["nt"] - 1, pol=1, m=s["M"] - 1, l=s["L"] - 1,
                n0=s["N"] - 1)
    first = {a: 0 for a in ONE_HOT_AXES}
    idx = [first, last]
    for a in ONE_HOT_AXES:
        idx.append(dict(first, **{a: last[a]}))
        idx.append(dict(last, **{a: 0}))
    return [(S, i) for S in (16, 5) for i in idx]


def one_hot_expected(S, i, l_min=0):
    """-> (rx, i, pol, n) of the single 1 of y, or None when block m does not own that sample"""
    s = ONE_HOT_SHAPE
    n = i["n0"] + l_min + i["l"]
    if not 0 <= n < s["n_out"] or min(n // S, s["M"] - 1) != i["m"]:
        return None
    return (i["rx"], i["i"], i["pol"], n)


def one_hot_tensors(i):
    s = ONE_HOT_SHAPE
    h = np.zeros((s["nrx"], s["ntx"], s["nr"], s["nt"], 2, s["M"], s["L"]), np.complex64)
    x = np.zeros((s["ntx"], s["nt"], s["N"]), np.complex64)
    h[i["rx"], i["tx"], i["i"], i["j"], i["pol"], i["m"], i["l"]] = 1
    x[i["tx"], i["j"], i["n0"]] = 1
    return h, x


# ---------------------------------------------------------------------------------------------- real-valued

# R = 24 complex rows, K = 2 * 3 * 37 complex reductions, N_out = 200; every output has a term: N + L - 1 >= N_out
REAL_SHAPE = dict(nrx=4, nr=3, ntx=2, nt=3, L=37, N=180, n_out=200, l_min=0)
REAL_BLOCKS = {MFMA: (48, 5), GENERAL: (41, 5)}   # (S, M)


def plant_normal(shape, M, seed):
    rng = np.random.RandomState(seed)
    hs = (shape["nrx"], shape["ntx"], shape["nr"], shape["nt"], 2, M, shape["L"])
    xs = (shape["ntx"], shape["nt"], shape["N"])
    h = rng.standard_normal(hs) + 1j * rng.standard_normal(hs)
    x = rng.standard_normal(xs) + 1j * rng.standard_normal(xs)
    return h.astype(np.complex64), x.astype(np.complex64)
