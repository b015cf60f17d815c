"""The walk of the trace and record kernels -- closest_hit_words over HRT_STAGED_TEST, csrc/hrt_kernels.hip -- on
PLANTED rays, through its test entry (hrt_selftest_math fn 11, include/hrt_device.h: a ray, a kind and up to eight
triangles given inline), against a float32 transcription of the reference's scan (closest_hit_plain, i.e.
src/compute_paths.c's sequence: NumPy single operations, nothing contracted).  The winning row and the bits of its
distance (kind 0) or the one-metre decision (kind 2) must match exactly.

The staged test skips the u and v divisions where the hit is CERTAIN (numerators inside [0, a] with a 2^-20 margin on
their sum, see the comment above the macro), and a shadow walk (kind 2) skips the distance division too: it carries
its best candidate as the pair (Nt', a), orders candidates by cross products and divides only in a band of 2^-20
around equality, around dist = eps and where a product leaves its range.  The planted set sits where the certificate,
the stage rejections, the band and the take rule change their answer:

  * rays through the three vertices; along and across the edge two triangles share, in both orientations (det < 0 too);
  * u, v and u + v at 0 and 1 and their float neighbours (and at -eps, 1 + eps and theirs);
  * two coplanar overlapping triangles at equal distance, both orders of their original indices;
  * two hits whose distances differ by 0, 1 and 2 ulp, nearer one first and second;
  * a hit at t = 1 and its neighbours (kind 2); t at eps and its neighbours; |det| at eps and its neighbours;
  * numerators at the edges of the certificate's exponent range: |det| at and beyond 2^126, 2^127 and overflowing,
    denormal numerators;
  * lanes without a ray, and a partial last wave.

The device decides per WAVE (it runs the exact sequence for a row as soon as one lane is not certain), so every planted
item runs twice: alone in a wave of its own (at a lane that moves with the item), where the path taken is the item's
own band, and packed with the others and with random rays, where bands mix.

Every GPU step is a process of its own under a time limit; after a step that failed, none is started again."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 120
F = np.float32
NO_HIT = 0xFFFFFFFF
NO_RAY = 7             # a kind that is neither 0 nor 2: the lane carries no ray
ITEM = 168             # floats per item: 8 + 8 rows of 20
EPS = F(1.1920928955078125e-07)
ONE_EPS = F(1.00000011920928955078125)
# the constants of the staged test, formed in float32 like the kernel's constexpr floats
K1 = EPS * (F(1) + F(2.0 ** -18))
K2 = F(1) + F(2.0 ** -20)
K3 = F(1) + F(2.0 ** -19)
K5 = EPS * (F(1) - F(2.0 ** -18))
CERT_W = F(1) - F(2.0 ** -20)
CERT_MAX_DET = F(2.0 ** 126)
K5H = EPS * (F(1) + F(2.0 ** -18))
PAIR_MAX = F(2.0 ** 120)
BAND = F(2.0 ** -20)   # the relative width of the near-tie band of two distances' cross products


def up(x, k=1):
    """float32 x moved k ulps (k < 0: down)"""
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


# ---------------------------------------------------------------- the reference's scan, float32 operation by operation
def _v(a):
    return [F(a[0]), F(a[1]), F(a[2])]


def sub3(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def dot3(a, b):   # inc/vec3.h: (x*x' + y*y') + z*z'
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def sign_corrected(x, det):
    return -x if np.signbit(det) else x


def reference_walk(o, d, tris):
    """tris: [(v1, e1, e2, orig)] in table order -> (who, best, bands): the lexicographic minimum of (distance, orig) over
    the rows the reference's test accepts -- its scan in `orig` order with a strict '<' -- and, per row, the band the
    staged test puts the ray in, computed from these float32 values alone."""
    o, d = _v(o), _v(d)
    best, who, who_o = F(1e9), NO_HIT, 0
    nt_b, a_b = F(1e9), F(1)   # the best candidate's (Nt', a), as a shadow walk carries it; no hit yet: quotient 1e9
    bands = []
    with np.errstate(all="ignore"):
        for j, (v1, e1, e2, orig) in enumerate(tris):
            v1, e1, e2 = _v(v1), _v(e1), _v(e2)
            pv = cross3(d, e2)
            det = dot3(e1, pv)
            s = sub3(o, v1)
            nu = dot3(s, pv)
            q = cross3(s, e1)
            nv = dot3(d, q)
            nt = dot3(e2, q)
            # the staged test's view of the row (a = |det|, numerators with det's sign taken out)
            a = np.abs(det)
            nu_s, nv_s, nt_s = sign_corrected(nu, det), sign_corrected(nv, det), sign_corrected(nt, det)
            rejected = bool((a < EPS) | (nu_s < -(K1 * a)) | (nu_s > K2 * a) | (nv_s < -(K1 * a)) |
                            ((nu_s + nv_s) > K3 * a) | (nt_s < K5 * a) | (nt_s > (best * a) * K2))
            certain = bool((nu_s >= 0) & (nv_s >= 0) & ((nu_s + nv_s) <= CERT_W * a) & (a <= CERT_MAX_DET))
            band = "rejected" if rejected else ("certain" if certain else "uncertain")
            # a shadow walk orders candidates by the products of (Nt', a) pairs and divides only in a band around equality,
            # around dist = eps, or where a product is out of range
            p_new, p_old = nt_s * a_b, nt_b * a
            in_play = not bool((a < EPS) | (nu_s < -(K1 * a)) | (nu_s > K2 * a) | (nv_s < -(K1 * a)) |
                               ((nu_s + nv_s) > K3 * a) | (nt_s < K5 * a) | (p_new > p_old * K2))
            pair_band = in_play and not bool((nt_s > K5H * a) & (p_new < p_old * CERT_W) & (p_old <= PAIR_MAX))
            # the reference's sequence
            hit = False
            if not (det > -EPS and det < EPS):
                u = nu / det
                if not (u < -EPS or u > ONE_EPS):
                    v = nv / det
                    w = u + v
                    if not (v < -EPS or w > ONE_EPS):
                        hit = True
                        dist = nt / det
                        tie = False
                        if who != NO_HIT and dist > EPS:
                            p_new, p_old = nt_s * a_b, nt_b * a
                            tie = bool((p_new >= p_old * (F(1) - BAND)) & (p_new <= p_old * (F(1) + BAND)))
                        if dist > EPS and (dist < best or (dist == best and orig < who_o)):
                            best, who, who_o, nt_b, a_b = dist, j, orig, nt_s, a
                        if tie:
                            band += "+near_tie"
            if in_play:
                band += "+pair_band" if pair_band else "+pair_clear"
            if band.startswith("uncertain"):
                band = band.replace("uncertain", "uncertain_hit" if hit else "uncertain_miss", 1)
            assert not (band.startswith("certain") and not hit), "the certificate holds on a row the reference rejects"
            bands.append(band)
    return who, best, bands


# ---------------------------------------------------------------- the planted set
def tri(v1, e1, e2, orig):
    return (tuple(v1), tuple(e1), tuple(e2), int(orig))


def unit(orig=0, z=0.0, scale=1.0, flip=False):
    """the triangle (0,0,z) (s,0,z) (0,s,z); flip: e1 and e2 exchanged, which changes det's sign (u and v exchange)"""
    e1, e2 = (scale, 0.0, 0.0), (0.0, scale, 0.0)
    return tri((0.0, 0.0, z), e2 if flip else e1, e1 if flip else e2, orig)


def planted():
    """[(tag, kind, o, d, tris)] -- for the unit triangle and d = (0, 0, -k): det = k, u = fl(fl(k x) / k),
    v = fl(fl(k y) / k), t = fl((o.z - z) / k)."""
    P = []
    half, one = F(0.5), F(1)
    hyp = tri((1.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (0.0, -1.0, 0.0), 1)   # shares the edge x + y = 1 with unit()
    downs = [(0.0, 0.0, -1.0), (0.0, 0.0, -3.0)]
    # through a vertex: straight down and from a slanted origin, from above and from below (det < 0)
    for vx, vy in ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0)):
        for dd in downs:
            P.append(("vertex", 0, (vx, vy, 1.0), dd, [unit(), hyp]))
        for oo in ((0.3, 0.2, 1.7), (-0.6, 1.4, -2.3)):
            o = _v(oo)
            P.append(("vertex_slant", 0, oo, tuple(F(c) - oc for c, oc in zip((vx, vy, 0.0), o)), [unit(), hyp]))
    # along the shared edge and across it, both orientations of both triangles, both sides of the plane
    for flip in (False, True):
        pair = [unit(0, flip=flip), hyp if not flip else tri((1.0, 1.0, 0.0), (0.0, -1.0, 0.0), (-1.0, 0.0, 0.0), 1)]
        for t in (0.0, 0.125, 0.3, 0.5, 0.7, 0.875, 1.0):
            x = F(t)
            for oz, dz in ((1.0, -1.0), (-1.0, 1.0), (1.0, -3.0)):
                P.append(("edge_along", 0, (x, one - x, oz), (0.0, 0.0, dz), pair))
                P.append(("edge_along", 0, (x, one - x, oz), (0.0, 0.0, dz), pair[::-1]))
        for k in range(-3, 4):
            for oz, dz in ((1.0, -1.0), (-1.0, 1.0), (1.0, -3.0)):
                P.append(("edge_across", 0, (up(half, k), up(half, k), oz), (0.0, 0.0, dz), pair))
                P.append(("edge_across", 2, (up(half, k), half, oz), (0.0, 0.0, dz), pair))
    # u, v at 0, -eps, 1, 1 + eps and their neighbours; u + v at 1, 1 + eps and theirs
    zero_side = [F(0), up(0, 1), up(0, -1), -EPS, up(-EPS, 1), up(-EPS, -1), -K1, up(-K1, 1), up(-K1, -1), F(1e-40), F(-1e-40)]
    one_side = [one, up(1, -1), up(1, 1), ONE_EPS, up(ONE_EPS, 1), up(1, 2), K2, up(K2, 1), up(K2, -1), CERT_W, up(CERT_W, 1),
                up(CERT_W, -1)]
    for dd in downs:
        for flip in (False, True):
            for c in zero_side + one_side:
                P.append(("u_edge", 0, (c, 0.25, 1.0), dd, [unit(flip=flip)]))
                P.append(("v_edge", 0, (0.25, c, 1.0), dd, [unit(flip=flip)]))
            for c in zero_side:
                P.append(("uv_zero", 0, (c, c, 1.0), dd, [unit(flip=flip)]))
            for k in range(-3, 4):   # u + v = 1 + k 2^-24 (k < 0) or 1 + k 2^-23: exact sums of exact quotients for det = 1
                P.append(("w_edge", 0, (half, up(half, 2 * k if k > 0 else k), 1.0), dd, [unit(flip=flip)]))
                P.append(("w_edge", 0, (up(F(0.25), k), F(0.75), 1.0), dd, [unit(flip=flip)]))
            for c in (CERT_W, up(CERT_W, 1), up(CERT_W, -1), up(CERT_W, 2), up(CERT_W, -2)):   # the certificate's own edge
                P.append(("cert_edge", 0, (half, c - half, 1.0), dd, [unit(flip=flip)]))
                P.append(("cert_edge", 2, (F(0.3), c - F(0.3), 1.0), dd, [unit(flip=flip)]))
    # two coplanar overlapping triangles at equal distance: the original index decides, in both orders
    big = tri((-1.0, -1.0, 0.0), (3.0, 0.0, 0.0), (0.0, 3.0, 0.0), 0)
    for oa, ob in ((0, 1), (1, 0), (5, 3), (3, 5)):
        for pair in ([unit(oa), unit(ob)], [unit(oa), big[:3] + (ob,)], [big[:3] + (oa,), unit(ob, flip=True)]):
            for kind in (0, 2):
                P.append(("coplanar_tie", kind, (0.25, 0.25, 1.0), (0.0, 0.0, -1.0), pair))
                P.append(("coplanar_tie", kind, (0.3, 0.2, 1.7), (-0.05, 0.05, -1.7), pair))
    # two hits 0, 1 and 2 ulp apart (t = 1 - z for d = (0, 0, -1)), nearer one first and second, both index orders
    for k in (0, 1, 2):
        z = -(up(1, k) - one)   # exact: -k 2^-23
        for first_near in (True, False):
            for oa, ob in ((0, 1), (1, 0)):
                near, far = unit(oa), unit(ob, z=float(z))
                pair = [near, far] if first_near else [far[:3] + (oa,), near[:3] + (ob,)]
                for kind in (0, 2):
                    P.append(("ulp_apart_%d" % k, kind, (0.25, 0.25, 1.0), (0.0, 0.0, -1.0), pair))
                    P.append(("ulp_apart_%d" % k, kind, (0.25, 0.25, 3.0), (0.0, 0.0, -3.0), pair))
    # a hit at t = 1 and its neighbours (the one-metre decision of a shadow walk); t at eps and its neighbours
    for k in range(-2, 3):
        for kind in (0, 2):
            P.append(("t_one", kind, (0.25, 0.25, up(1, k)), (0.0, 0.0, -1.0), [unit()]))
            P.append(("t_one", kind, (0.25, 0.25, up(3, k)), (0.0, 0.0, -3.0), [unit()]))
            P.append(("t_one", kind, (0.2, 0.3, 1.0), (0.1, 0.1, up(-1, k)), [unit(), unit(1, z=-0.5)]))
            P.append(("t_eps", kind, (0.25, 0.25, up(EPS, k)), (0.0, 0.0, -1.0), [unit()]))
            P.append(("t_eps", kind, (0.25, 0.25, up(K5, k)), (0.0, 0.0, -1.0), [unit()]))
            P.append(("t_eps", kind, (0.25, 0.25, up(3 * EPS, k)), (0.0, 0.0, -3.0), [unit(), unit(1, z=-0.5)]))
    # |det| at eps and its neighbours (d = (0, 0, -k): det = k), both signs
    for k in range(-2, 3):
        for sgn in (1.0, -1.0):
            P.append(("det_eps", 0, (0.25, 0.25, sgn), (0.0, 0.0, -sgn * up(EPS, k)), [unit()]))
            P.append(("det_eps", 0, (0.25, 0.25, sgn), (0.0, 0.0, -sgn * up(EPS, k)), [unit(flip=True), unit(1, z=-0.5)]))
    # the certificate's exponent range: det = s^2 k at 2^126 and its neighbours, 2^127, overflowing; denormal numerators
    s63 = 2.0 ** 63
    for kk in (one, up(1, 1), up(1, -1), F(2), F(4)):   # det = 2^126 k: the last certain one, beyond, 2^127, infinite
        for x, y in ((0.25, 0.25), (0.4, 0.4), (0.6, 0.6), (1.0, 0.0), (0.0, 0.0), (0.5, 0.5)):
            for kind in (0, 2):
                P.append(("det_huge", kind, (x * s63, y * s63, 1.0), (0.0, 0.0, -float(kk)), [unit(scale=s63), unit(1, z=-0.5)]))
    for x in (1e-40, 1e-45, 3e-39, 1.1754944e-38):
        for dd in downs + [(0.0, 0.0, -float(EPS))]:
            P.append(("denormal", 0, (x, x, 1.0), dd, [unit()]))
            P.append(("denormal", 0, (x, 0.25, 1.0), dd, [unit(flip=True)]))
    return P


def random_items(n, seed):
    """rays aimed at a point of one of eight random triangles (hits and near misses are common)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        T = int(rng.integers(1, 9))
        tris = []
        for j in range(T):
            v1 = rng.uniform(-5, 5, 3)
            tris.append(tri(v1, rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3), j))
        perm = rng.permutation(T)
        tris = [t[:3] + (int(perm[j]),) for j, t in enumerate(tris)]
        v1, e1, e2, _ = tris[int(rng.integers(0, T))]
        bu, bv = rng.uniform(-0.1, 1.1), rng.uniform(-0.1, 0.6)
        if i % 5 == 0:
            bu, bv = float(rng.integers(0, 2)), 0.0   # at a vertex
        elif i % 5 == 1:
            bv = 1.0 - bu                               # on the hypotenuse
        p = np.asarray(v1) + bu * np.asarray(e1) + bv * np.asarray(e2)
        o = rng.uniform(-8, 8, 3)
        out.append(("random", (0, 2)[i % 2], tuple(o), tuple((p - o) * rng.uniform(0.5, 2.0)), tris))
    return out


def pack(items, lanes):
    """items [(tag, kind, o, d, tris)] at the lane positions `lanes` of an array of max(lanes) + 1 items; every other
    position is a lane without a ray -> float32 [n_items][168]"""
    n = max(lanes) + 1
    x = np.zeros((n, ITEM), np.float32)
    xb = x.view(np.uint32)
    xb[:, 6] = NO_RAY
    with np.errstate(over="ignore"):
        for pos, (_, kind, o, d, tris) in zip(lanes, items):
            x[pos, 0:3], x[pos, 3:6] = _v(o), _v(d)
            xb[pos, 6], xb[pos, 7] = kind, len(tris)
            for j, (v1, e1, e2, orig) in enumerate(tris):
                r = 8 + 20 * j
                x[pos, r:r + 3], x[pos, r + 3:r + 6], x[pos, r + 6:r + 9] = _v(v1), _v(e1), _v(e2)
                xb[pos, r + 19] = orig
    return x


_cache = {}


def the_set():
    """the planted items, the random ones and the reference's answers, computed once"""
    if not _cache:
        P, R = planted(), random_items(300, seed=23)
        _cache["planted"], _cache["random"] = P, R
        _cache["ref"] = [reference_walk(o, d, tris) for _, _, o, d, tris in P + R]
    return _cache["planted"], _cache["random"], _cache["ref"]


def expected(items, refs):
    want = np.zeros((len(items), 2), np.uint32)
    for i, ((_, kind, _, _, _), (who, best, _)) in enumerate(zip(items, refs)):
        want[i, 0] = who
        want[i, 1] = (1 if best <= F(1) else 0) if kind == 2 else np.asarray(best, np.float32).view(np.uint32)
    return want


# ---------------------------------------------------------------- without a GPU
def test_the_planted_set_reaches_every_band():
    """From the transcription alone: some planted ray's row is certain, some is uncertain and hits, some is uncertain and
    misses, some is a near tie of two accepted distances; the tags the module text lists are all present; and wherever
    the certificate holds on a row the stages do not reject, the reference accepts the row (asserted inside
    reference_walk for every row of the planted and the random set)."""
    P, R, refs = the_set()
    seen = set()
    for (tag, kind, _, _, _), (_, _, bands) in zip(P, refs[:len(P)]):
        for b in bands:
            seen.update(b.split("+"))
    assert {"certain", "uncertain_hit", "uncertain_miss", "near_tie", "rejected"} <= seen, seen
    # the shadow walks' pair ordering: among the kind-2 items, rows decided by the products alone and rows in its band
    shadow = set()
    for (tag, kind, _, _, _), (_, _, bands) in zip(P, refs[:len(P)]):
        if kind == 2:
            for b in bands:
                shadow.update((x, tag) for x in b.split("+") if x.startswith("pair_"))
    assert {x for x, _ in shadow} == {"pair_band", "pair_clear"}, shadow
    for tag in ("coplanar_tie", "ulp_apart_0", "ulp_apart_1", "ulp_apart_2", "t_eps", "det_huge"):
        assert ("pair_band", tag) in shadow, tag
    tags = {p[0] for p in P}
    assert {"vertex", "edge_along", "edge_across", "u_edge", "v_edge", "w_edge", "coplanar_tie", "ulp_apart_0", "ulp_apart_1",
            "ulp_apart_2", "t_one", "t_eps", "det_eps", "det_huge", "denormal"} <= tags
    # each band also occurs with det < 0, and the one-metre decision goes both ways among the shadow items
    metre = {bool(best <= F(1)) for (_, kind, _, _, _), (who, best, _) in zip(P, refs) if kind == 2 and who != NO_HIT}
    assert metre == {True, False}
    rand_bands = set()
    for _, _, bands in refs[len(P):]:
        rand_bands.update(b.split("+")[0] for b in bands)
    assert {"certain", "rejected"} <= rand_bands, rand_bands


def test_the_transcription_on_rays_worked_by_hand():
    """unit triangle, straight down: u = x, v = y, t = o.z; outside: no hit; equal distances: the lower original index"""
    who, best, bands = reference_walk((0.25, 0.25, 2.0), (0, 0, -1), [unit()])
    assert who == 0 and best == F(2) and bands == ["certain+pair_clear"]
    who, best, _ = reference_walk((0.75, 0.75, 2.0), (0, 0, -1), [unit()])
    assert who == NO_HIT and best == F(1e9)
    who, best, _ = reference_walk((0.25, 0.25, 2.0), (0, 0, -1), [unit(4), unit(2)])
    assert who == 1 and best == F(2)
    who, best, bands = reference_walk((0.5, 0.5, 2.0), (0, 0, -1), [unit()])   # on the hypotenuse: a hit, not certain
    assert who == 0 and bands == ["uncertain_hit+pair_clear"]


# ---------------------------------------------------------------- on the GPU
_CHILD = """
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from hermespy_rt_amd import lib
L = lib.load()
x = np.ascontiguousarray(np.load(sys.argv[1]))
out = np.zeros_like(x)
f32p = C.POINTER(C.c_float)
lib.check(L.hrt_selftest_math(0, 11, x.ctypes.data_as(f32p), out.ctypes.data_as(f32p), x.size), "hrt_selftest_math")
np.save(sys.argv[2], out[:, :2].copy())
""" % REPO

_failed = []   # the first GPU step that failed: nothing is started after it


def device_walk(tmp_path, name, x):
    """fn 11 over the items x [n][168] in a process of its own -> uint32 [n][2] (row, distance bits or decision)"""
    if _failed:
        pytest.fail("not started: GPU step %s failed before" % _failed[0])
    src, dst = str(tmp_path / (name + "_in.npy")), str(tmp_path / (name + "_out.npy"))
    np.save(src, x)
    try:
        p = subprocess.run([sys.executable, "-c", _CHILD, src, dst], capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _failed.append(name + " (time limit)")
        raise
    if p.returncode != 0:
        _failed.append("%s (exit %d)" % (name, p.returncode))
        pytest.fail("%s: exit %d\n%s" % (name, p.returncode, p.stderr[-2000:]))
    out = np.load(dst)
    assert out.shape == (x.shape[0], 2) and out.dtype == np.float32
    return out.view(np.uint32)


def report(items, refs, got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    lines = ["%d of %d items differ" % (bad.size, len(items))]
    for i in bad[:40]:
        tag, kind, o, d, tris = items[i]
        lines.append("%s kind %d o %r d %r: got row %#x word %#010x, want row %#x word %#010x, bands %s" % (
            tag, kind, tuple(map(float, o)), tuple(map(float, d)), got[i, 0], got[i, 1], want[i, 0], want[i, 1], refs[i][2]))
    tags = sorted({items[i][0] for i in bad})
    lines.append("tags that fail: " + ", ".join(tags))
    return "\n".join(lines)


@pytest.mark.gpu
def test_each_planted_ray_alone_in_its_wave(tmp_path):
    """one item per wave, at lane (5 i) mod 64, the other 63 lanes without a ray: the path taken is the item's own"""
    P, _, refs = the_set()
    lanes = [64 * i + (5 * i) % 64 for i in range(len(P))]
    got_all = device_walk(tmp_path, "alone", pack(P, lanes))
    got, want = got_all[lanes], expected(P, refs[:len(P)])
    print("alone: %d planted items, %d differ" % (len(P), int((got != want).any(axis=1).sum())))
    assert np.array_equal(got, want), report(P, refs, got, want)
    rest = np.ones(got_all.shape[0], bool)
    rest[lanes] = False
    assert (got_all[rest, 0] == NO_HIT).all()   # a lane without a ray reports no hit


@pytest.mark.gpu
def test_planted_and_random_rays_packed(tmp_path):
    """all items side by side, every seventh position a lane without a ray, a partial last wave: a wave's lanes are in
    different bands and walk the union of their rows"""
    P, R, refs = the_set()
    items = P + R
    lanes, pos = [], 0
    for _ in items:
        if pos % 7 == 3:
            pos += 1
        lanes.append(pos)
        pos += 1
    if (lanes[-1] + 1) % 64 == 0:   # (keep the last wave partial)
        lanes[-1] += 1
    assert (lanes[-1] + 1) % 64 != 0
    got_all = device_walk(tmp_path, "packed", pack(items, lanes))
    got, want = got_all[lanes], expected(items, refs)
    print("packed: %d items in %d positions, %d differ" % (len(items), lanes[-1] + 1, int((got != want).any(axis=1).sum())))
    assert np.array_equal(got, want), report(items, refs, got, want)
    rest = np.ones(got_all.shape[0], bool)
    rest[lanes] = False
    assert (got_all[rest, 0] == NO_HIT).all()
