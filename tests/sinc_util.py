"""The sinc weights of the taps families (csrc/hrt_sinc.h: sinc_prep, sinc_tap), tap by tap.  Plain numpy, no device.

    sinc_ref      the float64 reference of the documented contract
    sinc_emulate  a float32 restatement of the header, every rounding where the header has it, with switchable
                  mutations (MUTATIONS) for the negative controls of tests/test_sinc_design.py
    cases         the delay classes, tau constructed so that the class is certain in double
    check         |got - ref| <= B 2^-24 |ref| + 2^-126, exact where the reference is exactly 0 or 1
    phase_*       the same for the carrier / Doppler phase factor of a record (the bound P)

tests/test_gpu_sinc_weights.py reads the weights off the device: with a single live record of amplitude 1 and phase 0
in a link, the output tap is the kernel's weight bit for bit (tests/planted.py plant_single)."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24                 # the unit of every error figure here: half an ulp of a float32 in [1, 2)
TINY = 2.0 ** -126             # the smallest normal float32: the kernels may flush what lies below it
CLAMP = 2.0 ** 26              # sinc_prep clamps rint(x) to +-2^26
TAP_MAX = 1 << 24              # validated tap indices: -2^24 <= l_min, l_min + L <= 2^24

# The bound of check() on a weight of the device, in units of 2^-24 |w|.
#   floor   the faithful emulation (a correctly rounded sinpi and reciprocal) against sinc_ref over every case of
#           cases(): 3.87 units (tests/test_sinc_design.py measures it and asserts ceil(floor) == FLOOR_CEIL)
#   + 1     v_rcp_f32 is accurate to 1 ulp, not 1/2
#   + 3     sinpif taken at up to 2 ulp, not 1/2: 1.5 ulp more = 3 units (the ROCm installation carries no accuracy
#           table for OCML's sinpif that would say otherwise)
#   + 2     slack
# The device measures 4.39 units at most (tests/test_gpu_sinc_weights.py prints it per class).
FLOOR_CEIL = 4
B = FLOOR_CEIL + 6

# The bound on a record's term with the phase on, a cis(nu t - fc tau) w: (B + P) 2^-24 |a| |w|.
#   floor   the phase factor alone: the FP64 phase as the device may form it (two roundings, or either product fused
#           into the difference), its half-revolution argument rounded to f32 and a correctly rounded sincospi,
#           against the reference's cis over the phase cases: 1.95 units (pi / 2 for the argument, 1 / sqrt(2) for
#           sincospi, and the FP64 roundings), measured by tests/test_sinc_design.py (asserted: ceil(floor + 1/2) ==
#           PHASE_FLOOR_CEIL); the + 1/2 is the one rounding of the product (a cis) w, a = 1 and 1/2 being exact
#   + 3     sincospif at up to 2 ulp per component, as for sinpif above
# (the slack of 2 units is in B already)
PHASE_FLOOR_CEIL = 3
P = PHASE_FLOOR_CEIL + 3

MUTATIONS = ("switch_1e3", "x_float", "tie_away", "no_clamp", "parity_of_k", "c_remainder", "rcp_12bit", "scaled")


def _f32(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float32)


def _grid(tau32, l):
    tau32 = np.asarray(tau32, np.float32).reshape(-1)
    l = np.asarray(l, np.int64).reshape(-1)
    return tau32[:, None], l[None, :]


# ------------------------------------------------------------------ the reference
def sinc_ref(fs, tau32, l):
    """sinc(l - x), x the float64 product fs * float64(tau32), as float64 [len(tau32), len(l)]: with n = rint(x),
    f = x - n (exact), w = -(-1)^(l - n) sin(pi f) / (pi ((l - n) - f)); exactly 1 where l - x == 0 and exactly 0
    where x is an integer and l != x (every x >= 2^53 among them)"""
    tau, l = _grid(tau32, l)
    x = np.float64(fs) * tau.astype(np.float64)
    n = np.rint(x)
    f = x - n
    dn = l.astype(np.float64) - n              # exact below 2^53; beyond it f == 0 and the weight is 0 or 1
    odd = np.fmod(dn, 2.0) != 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.sin(np.pi * f) / (np.pi * (dn - f))
    w = np.where(odd, w, -w)
    lx = l.astype(np.float64) - x
    return np.where(lx == 0.0, 1.0, np.where(f == 0.0, 0.0, w))


def sinc_mp(fs, tau32, l, bits=200):
    """sinc_ref's contract in mpmath at `bits` bits, from the same double x (a list of lists of mpf)"""
    import mpmath
    tau, l = _grid(tau32, l)
    x = np.float64(fs) * tau.astype(np.float64)
    out = []
    with mpmath.workprec(bits):
        for xi in x[:, 0]:
            xm = mpmath.mpf(float(xi))
            row = []
            for li in l[0]:
                d = mpmath.mpf(int(li)) - xm
                row.append(mpmath.mpf(1) if d == 0 else mpmath.sinpi(d) / (mpmath.pi * d))
            out.append(row)
    return out


# ------------------------------------------------------------------ the header, restated in float32
def _sinpi_f32(f32):
    """a correctly rounded sinpif of |f| <= 1/2 (from float64)"""
    return np.sin(np.pi * f32.astype(np.float64)).astype(np.float32)


def _rcp_f32(d, bits=24):
    with np.errstate(divide="ignore"):
        r = (1.0 / d.astype(np.float64))
    if bits < 24:
        m, e = np.frexp(r)
        r = np.ldexp(np.rint(np.ldexp(m, bits)), e - bits)
    return _f32(r)


def _round_away(x):
    return np.copysign(np.floor(np.abs(x) + 0.5), x)


def _wrap_i32(n):
    """(int32_t) of a double as a wrapping conversion (beyond 2^62: 0)"""
    ok = np.abs(n) < 2.0 ** 62
    i = np.where(ok, n, 0.0).astype(np.int64)
    return ((i + (1 << 31)) % (1 << 32)) - (1 << 31)


def sinc_emulate(fs, tau32, l, **mutations):
    """sinc_tap(l, sinc_prep(fs, tau32)) in numpy, float32 [len(tau32), len(l)], every rounding where the header has
    it; sinpi and the reciprocal correctly rounded.  Mutations (keyword = True), the negative controls:
        switch_1e3   the 1e-4 switch at 1e-3
        x_float      x = (float)fs * tau in float32
        tie_away     the parity of n from rint's tie resolved away from zero (f as the header has it)
        no_clamp     k = (int32_t)n wrapped, r = x - n, l - k a wrapped int32
        parity_of_k  the parity of the clamped k instead of n
        c_remainder  the sign of l from l % 2 == 1 with C's remainder (negative odd l count as even)
        rcp_12bit    a reciprocal good to 12 bits
        scaled       the weight times 1 + 2^-19"""
    bad = set(mutations) - set(MUTATIONS)
    assert not bad, bad
    mut = {k: bool(mutations.get(k)) for k in MUTATIONS}
    tau, l = _grid(tau32, l)
    if mut["x_float"]:
        with np.errstate(over="ignore"):
            x = (np.float32(fs) * tau).astype(np.float64)
    else:
        x = np.float64(fs) * tau.astype(np.float64)
    n = np.rint(x)
    k = n if mut["no_clamp"] else np.clip(n, -CLAMP, CLAMP)
    pn = _round_away(x) if mut["tie_away"] else (k if mut["parity_of_k"] else n)
    h = 0.5 * pn
    with np.errstate(invalid="ignore"):   # (x_float: the float32 product may be inf)
        s = _sinpi_f32(_f32(x - n)) * np.float32(0.318309886183790672)
        r = _f32(x - k)
    c = np.where(h != np.floor(h), s, -s)
    if mut["no_clamp"]:
        lk = _wrap_i32(l - _wrap_i32(k))
    else:
        lk = l - k.astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = lk.astype(np.float32) - r
        lodd = (np.fmod(l, 2) == 1) if mut["c_remainder"] else ((l & 1) == 1)
        cl = np.where(lodd, -c, c)
        w = cl * _rcp_f32(d, 12 if mut["rcp_12bit"] else 24)
        w = np.where(np.abs(d) < np.float32(1e-3 if mut["switch_1e3"] else 1e-4), np.float32(1.0), w)
        if mut["scaled"]:
            w = w * np.float32(1.0 + 2.0 ** -19)
    return w.astype(np.float32)


# ------------------------------------------------------------------ the check
def check(got, fs, tau32, l, B, ref_scale=1.0, what=""):
    """|got - ref| <= B 2^-24 |ref| + 2^-126 for got [len(tau32), len(l)] against sinc_ref (times ref_scale: the
    negative controls); got == ref where the reference is exactly 0 or 1 (either sign of zero); everything finite.
    Returns the largest |got - ref| / (2^-24 |ref|) seen (over the weights above 2^-100, where 2^-126 is nothing)."""
    ref = sinc_ref(fs, tau32, l)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    assert np.isfinite(got).all(), "%s: %d weights not finite" % (what, (~np.isfinite(got)).sum())
    exact = (ref == 0.0) | (ref == 1.0)
    ref = ref * ref_scale
    err = np.abs(got - ref)
    bad = np.where(exact, got != ref, err > B * U * np.abs(ref) + TINY)
    if bad.any():
        tau, lg = _grid(tau32, l)
        x = np.broadcast_to(np.float64(fs) * tau.astype(np.float64), ref.shape)
        ll = np.broadcast_to(lg, ref.shape)
        lines = ["  x = %.17g  l = %d: got %.9g want %.17g (%.1f units)"
                 % (x[ix], ll[ix], got[ix], ref[ix], err[ix] / max(U * abs(ref[ix]), 1e-300))
                 for ix in map(tuple, np.argwhere(bad)[:8])]
        raise AssertionError("%s: %d of %d weights outside %g 2^-24 |w| (fs = %.17g):\n%s"
                             % (what, bad.sum(), bad.size, B, fs, "\n".join(lines)))
    big = np.abs(ref) > 2.0 ** -100
    return float((err[big] / (U * np.abs(ref[big]))).max(initial=0.0))


# ------------------------------------------------------------------ the delay classes
def _tau_of(x, fs):
    return (np.asarray(x, np.float64) / fs).astype(np.float32)


def _generic(fs, xs, lo, hi, min_f=0.01):
    """tau32 with x = fs tau in (lo, hi) and a fraction of at least min_f, the first candidates of xs that qualify"""
    tau = _tau_of(xs, fs)
    x = np.float64(fs) * tau.astype(np.float64)
    f = x - np.rint(x)
    return tau[(x > lo) & (x < hi) & (np.abs(f) >= min_f)]


def cases():
    """[(class, fs, tau32[<= 48], [(l_min, L), ...])]: every delay of an entry is evaluated at every window of it.
    L in {1, 16, 17, 80}: the 16-tap column tiles and their ragged edge; one window of every class lies 10^3 to 10^6
    taps from the delays.  design_errors() proves the class of every delay in double."""
    rng = np.random.default_rng(20250)
    T24 = TAP_MAX
    out = []
    # a. generic fractions, x in [5, 500)
    for fs in (122.88e6, 1e9):
        tau = _generic(fs, rng.uniform(5.0, 500.0, 60), 5.0, 500.0, 1e-3)[:40]
        out.append(("a", fs, tau, [(0, 80), (190, 17), (400, 16), (499, 1), (300, 80), (100000, 16), (-1000, 17)]))
    # b. half-integers: rint ties to the even neighbour, below and above
    n = np.array([0, 1, 2, 3, 6, 7, 100, 101, (1 << 20), (1 << 20) + 1, (1 << 23) - 2, (1 << 23) - 1], np.float64)
    out.append(("b", 2.0 ** 30, _tau_of(n + 0.5, 2.0 ** 30),
                [(0, 16), (-3, 17), (95, 16), ((1 << 20) - 8, 17), ((1 << 23) - 40, 80), (-100000, 16), (3, 1)]))
    # c. the 1e-4 switch: f = +-n 2^-20 exactly, n on both sides of 105 (and of 1049: a switch moved to 1e-3)
    n = np.array([90, 100, 104, 105, 106, 110, 120, 200, 400, 700, 900, 1000, 1040, 1048, 1049, 1100], np.float64)
    for sg in (1.0, -1.0):
        fs = 2.0 ** 30 + sg * 2.0 ** 10
        out.append(("c", fs, _tau_of(n, 2.0 ** 30),
                    [(80, 80), (190, 17), (395, 16), (700, 1), (896, 17), (1000, 80), (1100, 1), (100000, 16)]))
    # d. tiny fractions: f = +-n 2^-30 and +-n 2^-40 exactly
    n = np.array([1, 3, 100, 1001, 4095], np.float64)   # (n (2^40 + 1) is exact in double)
    for eps in (1.0, -1.0, 2.0 ** -10, -2.0 ** -10):
        out.append(("d", 2.0 ** 30 + eps, _tau_of(n, 2.0 ** 30),
                    [(0, 16), (90, 17), (1000, 16), (4030, 80), (-100000, 1), (200000, 17)]))
    # e. exact integers, large n: exactly 1 and +-0
    n = (1 << 20) + np.arange(8, dtype=np.float64)
    out.append(("e", 2.0 ** 30, _tau_of(n, 2.0 ** 30),
                [((1 << 20) - 4, 16), (1 << 20, 1), ((1 << 20) - 40, 80), (0, 17)]))
    # f. negative delays (the rint tie and the parity of a negative n)
    x = np.array([-0.3, -2.5, -3.5, -100.25, -1.5, -7.75])
    for fs in (2.0 ** 30, 1e9):
        out.append(("f", fs, _tau_of(x, fs), [(-8, 16), (-5, 17), (-110, 16), (-40, 80), (-10000, 16), (1000, 1)]))
    # g. tau = 0 and denormal tau
    tau = np.array([0, 0x80000000, 1, 0x80000001, 71362, 0x007FFFFF, 0x807FFFFF], np.uint32).view(np.float32)
    for fs in (2.0 ** 30, 1e9):
        out.append(("g", fs, tau, [(0, 1), (-8, 17), (0, 16), (-40, 80), (1000, 16)]))
    # h. x just below 2^24: windows that end at the validated limit l_min + L = 2^24
    for fs in (122.88e6, 1e9):
        tau = _generic(fs, T24 - rng.uniform(1.0, 90.0, 40), T24 - 100.0, T24)[:24]
        out.append(("h", fs, tau, [(T24 - 80, 80), (T24 - 16, 16), (T24 - 17, 17), (T24 - 1, 1), (T24 - 100000, 16)]))
    # i. x in (2^24, 2^26): l - k is no longer exact in float32
    xs = np.concatenate([T24 + rng.uniform(1.0, 200.0, 10), rng.uniform(T24, CLAMP, 20), CLAMP - rng.uniform(1, 90, 10)])
    out.append(("i", 1e9, _generic(1e9, xs, T24, CLAMP)[:32],
                [(T24 - 80, 80), (T24 - 17, 17), (0, 16), (-T24, 16), (T24 - 1, 1)]))
    # j. past the clamp: x in (2^26, 2^27] and near 1e12 (fractions: fs = 1e9) ...
    xs = np.concatenate([CLAMP + rng.uniform(1.0, 2000.0, 12), rng.uniform(CLAMP, 2 * CLAMP, 16),
                         2 * CLAMP - rng.uniform(1, 90, 6), 1e12 + rng.uniform(-1e9, 1e9, 16)])
    wj = [(-T24, 16), (-T24, 80), (-8, 17), (0, 1), (T24 - 80, 80), (T24 - 17, 17)]
    out.append(("j", 1e9, _generic(1e9, xs, CLAMP, 2e12)[:44], wj))
    # ... and x an integer >= 2^53, up to fs tau > 3.5e38, where the float32 remainder x - k overflows
    tau = np.array([2.0 ** 23, 2.0 ** 24, 1e10, -1e10, 2.0 ** 60, 3.3e38, -3.3e38], np.float32)
    out.append(("j", 2.0 ** 30, tau, wj))
    return out


CLASSES = tuple("abcdefghij")


def design_errors(all_cases=None):
    """what is wrong with cases() (empty: nothing): every class as the issue defines it, proved in double"""
    errs = []
    seen = {c: [] for c in CLASSES}
    for cls, fs, tau, windows in cases() if all_cases is None else all_cases:
        x = np.float64(fs) * tau.astype(np.float64)
        n = np.rint(x)
        f = x - n
        seen[cls].append((fs, x, n, f))
        if not (0 < tau.size <= 48 and tau.dtype == np.float32):
            errs.append("%s: 1 .. 48 float32 delays per entry" % cls)
        Ls = {L for _, L in windows}
        if not Ls <= {1, 16, 17, 80} or not ({16, 17} & Ls):
            errs.append("%s: window lengths %s" % (cls, sorted(Ls)))
        if any(lo < -TAP_MAX or lo + L > TAP_MAX for lo, L in windows):
            errs.append("%s: a window outside +-2^24" % cls)
        far = [min(np.abs(x - lo).min(), np.abs(x - (lo + L - 1)).min()) for lo, L in windows]
        if not any(1e3 <= d for d in far):
            errs.append("%s: no far window" % cls)
        ok = {"a": ((x >= 5) & (x < 500) & (f != 0)).all(),
              "b": (np.abs(f) == 0.5).all() and (np.fmod(np.floor(x), 2) == 0).any()
              and (np.fmod(np.floor(x), 2) != 0).any(),
              "c": (np.abs(f) == n * 2.0 ** -20).all() and (np.abs(f) < 1e-4).any()
              and ((np.abs(f) > 1e-4) & (np.abs(f) < 1.9e-4)).any() and (np.abs(f) > 6.5e-4).any(),
              "d": ((np.abs(f) == n * 2.0 ** -30) | (np.abs(f) == n * 2.0 ** -40)).all(),
              "e": ((f == 0) & (x >= 2 ** 20)).all(),
              "f": (x < 0).all(),
              "g": (np.abs(tau) < TINY).all() and (tau == 0).any() and (tau != 0).any(),
              "h": ((x > TAP_MAX - 100) & (x < TAP_MAX) & (f != 0)).all()
              and any(lo + L == TAP_MAX for lo, L in windows),
              "i": ((x > TAP_MAX) & (x < CLAMP) & (f != 0)).all(),
              "j": (np.abs(x) > CLAMP).all()}[cls]
        if not ok:
            errs.append("%s: a delay outside its class (fs = %r)" % (cls, fs))
    for cls, got in seen.items():
        if not got:
            errs.append("%s: no entry" % cls)
    xj = np.concatenate([x for _, x, _, _ in seen["j"]])
    nj = np.concatenate([n for _, _, n, _ in seen["j"]])
    fj = np.concatenate([f for _, _, _, f in seen["j"]])
    inner = (xj > CLAMP) & (xj <= 2 * CLAMP) & (fj != 0)
    if not ((inner & (np.fmod(nj, 2) == 0)).any() and (inner & (np.fmod(nj, 2) != 0)).any()):
        errs.append("j: both parities of n in (2^26, 2^27]")
    if not (((np.abs(xj - 1e12) < 2e9) & (fj != 0)).any() and (np.abs(xj) >= 2.0 ** 53).any()
            and (np.abs(xj) > 3.5e38).any()):
        errs.append("j: near 1e12, >= 2^53 and past the float32 range")
    if not ({1e9, 122.88e6} <= {fs for fs, _, _, _ in seen["a"]}):
        errs.append("a: fs = 122.88e6 and 1e9")
    xf = np.concatenate([x for _, x, _, _ in seen["f"]])
    if not (np.isin([-2.5, -3.5], xf).all() and (np.abs(xf - np.rint(xf)) < 0.5).any()):
        errs.append("f: -2.5 and -3.5 (rint ties towards an even and away from an odd n) and a generic fraction")
    sg = [np.sign(f[f != 0][0]) for _, _, _, f in seen["c"]]
    if set(sg) != {1.0, -1.0}:
        errs.append("c: both signs of f")
    return errs


# ------------------------------------------------------------------ the phase factor of a record
def phase_ref(nu, t, fc, tau32):
    """cis(nu t - fc tau) in float64, the phase reduced as tests/planted.py cis does: [len(tau32), len(t)]"""
    from .planted import cis
    nu, t = np.asarray(nu, np.float64).reshape(-1, 1), np.asarray(t, np.float64).reshape(1, -1)
    tau = np.asarray(tau32, np.float32).astype(np.float64).reshape(-1, 1)
    return cis(nu * t - fc * tau)


def _fl(q):
    """a Fraction rounded to the nearest double"""
    return float(q)   # (Fraction.__float__ is correctly rounded)


def phase_emulate(nu, t, fc, tau32):
    """The phase factor as the kernels form it, complex128 of float32 parts, [3, len(tau32), len(t)]: the FP64 phase
    nu t - fc tau in the three ways a compiler may round it (both products rounded; either one fused into the
    difference), its fraction as (float)(2 (ph - rint(ph))), and a correctly rounded sincospi of that float."""
    nu, t = np.asarray(nu, np.float64).reshape(-1), np.asarray(t, np.float64).reshape(-1)
    tau = np.asarray(tau32, np.float32).astype(np.float64).reshape(-1)
    ph = np.empty((3, tau.size, t.size))
    for i in range(tau.size):
        b = Fraction(float(fc)) * Fraction(float(tau[i]))
        for m in range(t.size):
            a = Fraction(float(nu[i])) * Fraction(float(t[m]))
            ph[0, i, m] = _fl(a) - _fl(b)
            ph[1, i, m] = _fl(a - Fraction(_fl(b)))
            ph[2, i, m] = _fl(Fraction(_fl(a)) - b)
    h = (2.0 * (ph - np.rint(ph))).astype(np.float32).astype(np.float64)
    q = np.rint(2.0 * h)   # exact at the quarter revolutions, as sincospi is
    cs = np.where(2.0 * h == q, np.asarray([1.0, 0.0, -1.0, 0.0])[q.astype(np.int64) % 4], np.cos(np.pi * h))
    sn = np.where(2.0 * h == q, np.asarray([0.0, 1.0, 0.0, -1.0])[q.astype(np.int64) % 4], np.sin(np.pi * h))
    return cs.astype(np.float32).astype(np.float64) + 1j * sn.astype(np.float32).astype(np.float64)


PHASE_CLASSES = ("a", "c", "f", "h")


def by_link(tau32, nlinks):
    """the delays of a case dealt to nlinks links, link k the delay k mod len(tau32)"""
    return np.asarray(tau32, np.float32)[np.arange(nlinks) % len(tau32)]


def phase_inputs(nlinks):
    """the Doppler shifts (tests/planted.py NUS, link k the shift k mod 4) and the times t0 + m dt of the phase-on
    pass: t0 = -5 DT, dt = DT, num_times = 3"""
    from .planted import DT, NUS
    return np.asarray(NUS)[np.arange(nlinks) % len(NUS)], (-5.0 + np.arange(3)) * DT
