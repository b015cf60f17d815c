"""Planted queries for the candidate-mask tables (tests/test_gpu_candidates.py) -- pure numpy: no GPU, no oracle
library (the scene builders at the end use oracle.read_hrt, a file parser).

Every kernel that traces a ray on tables of at most 256 triangles takes its candidates from bit masks built once per
problem; the hot kernels walk the UNION over a wave, so a wrong entry hides behind the lane's neighbours.  The test
asks hrt_debug_candidates for ONE lane's own lookup on queries planted where the lookup decides something:

  * patch queries (modes 0 / 1): origins v1 + (fu / nu) e1 + (fv / nv) e2 + h n on every served triangle -- cell
    centres, cell borders, the strip outside the grid, +-hmax off the plane, the half of the parallelogram beyond
    the triangle -- plus NaN origins, rows past the table and every unserved triangle;
  * direction queries (modes 2 / 3): the Fibonacci set, every cube-map cell border, face edges and corners, axes.

A query's CLASS says what the lookup must do, computed here in float64 from the float32 origin that is emitted
(classes(): the bounds problem.c gives -- rounding of the cell coordinates < 1 / 64 of a cell, hball against hmax):
    MUST       on a served triangle, true cell coordinates at most 1 / 64 cell outside the grid, |h| <= hmax - 1e-5
    MUST_NOT   NaN origin, row past the table, unserved triangle, true coordinates more than ACCEPT + 1 / 64 outside
               the grid, or |h| >= hmax (1 + 2^-7) (aimed at hmax (1 + 2^-6); the other half of the margin is the
               rounding of the emitted origin and of the kernel's plane distance)
    EITHER     everything between: only soundness is asked
tests/test_candidates_design.py checks the classes with an independent formulation (least squares)."""
import numpy as np

RXT_N = 48                 # HRT_RXT_N
PATCH_ACCEPT = 0.03125     # HRT_PATCH_ACCEPT
PATCH_MAX_TRI = 256
MUST, EITHER, MUST_NOT = 2, 1, 0
BORDER = (0.0, 1.0 / 128, -1.0 / 128)                                  # and +-1 ulp, see _cell_offsets
OUTSIDE = (1.0 / 128, 1.0 / 64, 1.0 / 32 - 1.0 / 256, 1.0 / 32 + 1.0 / 256, 1.0 / 16)
IMG_FACTORS = (0.5, 0.9, 1.1, 2.0)
# kinds of a mode-1 query
IMG_BASE, IMG_ROT, IMG_REV = 0, 1, 2


def geometry(tri_vtx):
    """tri_vtx float32 [T][9] (v1 v2 v3, in the order of the table the queries address) -> float64 v1, e1, e2 (the
    float32 differences the product and the reference form), unit normal n (NaN for a degenerate triangle)."""
    t = np.asarray(tri_vtx, np.float32).reshape(-1, 3, 3)
    v1 = t[:, 0].astype(np.float64)
    e1 = (t[:, 1] - t[:, 0]).astype(np.float64)
    e2 = (t[:, 2] - t[:, 0]).astype(np.float64)
    c = np.cross(e1, e2)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = c / np.sqrt((c * c).sum(axis=1))[:, None]
    return dict(v1=v1, e1=e1, e2=e2, n=n)


def host_grid(tri_vtx, size=0.5):
    """The host's serving rule (csrc/host/problem.c patch_build) at patch edge `size`, in numpy: (nu, nv) per triangle,
    0 0 = refused (degenerate, or the rounding of the cell coordinates could exceed 1 / 64 of a cell)."""
    g = geometry(tri_vtx)
    t = np.asarray(tri_vtx, np.float32).reshape(-1, 3, 3)
    e1, e2 = g["e1"], g["e2"]
    pts = np.stack([g["v1"], g["v1"] + e1, g["v1"] + e2], axis=1).reshape(-1, 3)
    pts = pts[np.isfinite(pts).all(axis=1)]
    lo, hi = pts.min(axis=0).astype(np.float32).astype(np.float64), pts.max(axis=0).astype(np.float32).astype(np.float64)
    ext1 = (hi - lo).sum()
    u = 2.0 ** -24
    smax = ext1 + 1.0
    a11, a22, a12 = (e1 * e1).sum(axis=1), (e2 * e2).sum(axis=1), (e1 * e2).sum(axis=1)
    det = a11 * a22 - a12 * a12
    out = np.zeros((t.shape[0], 2), np.uint32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nrm = np.cross((t[:, 1] - t[:, 0]), (t[:, 2] - t[:, 0]))
        nrm = (nrm / np.sqrt((nrm * nrm).sum(axis=1, dtype=np.float32))[:, None]).astype(np.float32)
        ok = (det > 1e-30) & np.isfinite(det) & np.isfinite(nrm.sum(axis=1))
        nu = np.clip(np.ceil(np.sqrt(a11) / size), 1, 2048)
        nv = np.clip(np.ceil(np.sqrt(a22) / size), 1, 2048)
        g1 = (a22[:, None] * e1 - a12[:, None] * e2) / det[:, None] * nu[:, None]
        g2 = (a11[:, None] * e2 - a12[:, None] * e1) / det[:, None] * nv[:, None]
        lmax = np.maximum((g1 * g1).sum(axis=1), (g2 * g2).sum(axis=1))
        v1n = np.abs(g["v1"]).sum(axis=1)
        ok &= 16.0 * u * (smax + v1n) * np.sqrt(lmax) <= 1.0 / 64.0
    out[ok, 0] = nu[ok].astype(np.uint32)
    out[ok, 1] = nv[ok].astype(np.uint32)
    return out


def cell_coords(g, rows, nuv, o):
    """float64 cell coordinates (fu, fv) and plane distance h of origins o [n][3] on triangles `rows`: the dual basis of
    (e1, e2), what csrc/host/problem.c builds the definition rows from."""
    e1, e2 = g["e1"][rows], g["e2"][rows]
    a11, a22, a12 = (e1 * e1).sum(axis=1), (e2 * e2).sum(axis=1), (e1 * e2).sum(axis=1)
    det = a11 * a22 - a12 * a12
    s = np.asarray(o, np.float64) - g["v1"][rows]
    with np.errstate(invalid="ignore", divide="ignore"):
        fu = ((a22[:, None] * e1 - a12[:, None] * e2) * s).sum(axis=1) / det * nuv[rows, 0]
        fv = ((a11[:, None] * e2 - a12[:, None] * e1) * s).sum(axis=1) / det * nuv[rows, 1]
        h = (s * g["n"][rows]).sum(axis=1)
    return fu, fv, h


def classes(g, nuv, hmax, rows, o, num_tri):
    """MUST / EITHER / MUST_NOT of patch queries (row, float32 origin o), see the module text."""
    rows = np.asarray(rows, np.int64)
    n = rows.size
    cls = np.full(n, EITHER, np.int8)
    in_table = rows < num_tri
    r = np.where(in_table, rows, 0)
    served_tri = in_table & (nuv[r, 0] > 0)
    o64 = np.asarray(o, np.float32).astype(np.float64)
    nan = ~np.isfinite(o64).all(axis=1)
    fu, fv, h = cell_coords(g, r, nuv, np.where(nan[:, None], 0.0, o64))
    nu, nv = nuv[r, 0].astype(np.float64), nuv[r, 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        out_by = np.maximum.reduce([-fu, fu - nu, -fv, fv - nv])        # > 0: that far outside the grid, in cells
        must = served_tri & ~nan & (out_by <= 1.0 / 64) & (np.abs(h) <= float(hmax) - 1e-5)
        must_not = ~served_tri | nan | (out_by > PATCH_ACCEPT + 1.0 / 64) | (np.abs(h) >= float(hmax) * (1.0 + 2.0 ** -7))
    cls[must] = MUST
    cls[must_not] = MUST_NOT
    return cls


def _ulp_steps(x, k):
    """float32 x moved k ulps"""
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return float(x)


def _cell_offsets(i):
    """cell-unit coordinates around cell i of an axis: the centre, and both borders +- {0, 1 ulp, 1 / 128}"""
    out = [i + 0.5]
    for b in (i, i + 1):
        out += [b + x for x in BORDER] + [_ulp_steps(b, 1), _ulp_steps(b, -1)]
    return out


def pick_cells(nu, nv, rng, spread=2):
    """the four corner cells, the last cell (nu nv - 1) and `spread` random ones: [(iu, iv)]"""
    cells = [(0, 0), (nu - 1, 0), (0, nv - 1), (nu - 1, nv - 1)]
    last = nu * nv - 1
    cells.append((last % nu, last // nu))
    for _ in range(spread):
        cells.append((int(rng.integers(0, nu)), int(rng.integers(0, nv))))
    return sorted(set(cells))


def patch_queries(tri_vtx, nuv, hmax, seed=0, spread=2):
    """The patch queries of one table: dict(row [n] u32, o [n][3] float32, foot [n][3] float32 (the origin without its h),
    cell [n][2] (iu, iv aimed at; -1 where none), centre [n] bool (a cell-centre origin with h = 0), cls [n],
    tag [n] str).  tri_vtx in table-row order; nuv from hrt_debug_table_info."""
    rng = np.random.default_rng(seed)
    g = geometry(tri_vtx)
    T = g["v1"].shape[0]
    hmax = float(hmax)
    hs = [0.0, 1e-4, -1e-4, hmax * (1 - 2.0 ** -6), -hmax * (1 - 2.0 ** -6), hmax * (1 + 2.0 ** -6), -hmax * (1 + 2.0 ** -6)]
    row, FU, FV, H, cell, centre, tag = [], [], [], [], [], [], []

    def emit(j, fu, fv, h, c, t, is_centre=False):
        row.append(j); FU.append(fu); FV.append(fv); H.append(h); cell.append(c); centre.append(is_centre); tag.append(t)

    for j in range(T):
        nu, nv = int(nuv[j, 0]), int(nuv[j, 1])
        if nu == 0:
            # an unserved triangle: its centroid and a corner
            emit(j, 1.0 / 3, 1.0 / 3, 0.0, (-1, -1), "unserved")
            emit(j, 0.0, 0.0, 1e-4, (-1, -1), "unserved")
            continue
        k = 0
        for (iu, iv) in pick_cells(nu, nv, rng, spread):
            us, vs = _cell_offsets(iu), _cell_offsets(iv)
            for h in hs:   # the centre at every height
                emit(j, us[0], vs[0], h, (iu, iv), "centre", h == 0.0)
            for a, x in enumerate(us[1:]):   # every border offset of fu against the centre and one border offset of fv
                emit(j, x, vs[0], hs[k % 5], (iu, iv), "border_u"); k += 1
                emit(j, x, vs[1 + (a + k) % 10], hs[k % 5], (iu, iv), "border_uv"); k += 1
            for a, y in enumerate(vs[1:]):
                emit(j, us[0], y, hs[k % 5], (iu, iv), "border_v"); k += 1
                emit(j, us[1 + (a + k) % 10], y, hs[k % 5], (iu, iv), "border_uv"); k += 1
        # the strip outside the grid: four sides and four corners
        for dlt in OUTSIDE:
            mu, mv = rng.uniform(0.2, nu - 0.2), rng.uniform(0.2, nv - 0.2)
            for fu, fv in ((-dlt, mv), (nu + dlt, mv), (mu, -dlt), (mu, nv + dlt),
                           (-dlt, -dlt), (nu + dlt, -dlt), (-dlt, nv + dlt), (nu + dlt, nv + dlt)):
                emit(j, fu, fv, hs[k % 3], (-1, -1), "outside"); k += 1
    row = np.asarray(row, np.int64)
    nuf = np.where(nuv[row] > 0, nuv[row], 1).astype(np.float64)
    foot = g["v1"][row] + (np.asarray(FU) / nuf[:, 0])[:, None] * g["e1"][row] + (np.asarray(FV) / nuf[:, 1])[:, None] * g["e2"][row]
    with np.errstate(invalid="ignore"):
        nn = np.where(np.isfinite(g["n"][row]), g["n"][row], 0.0)
    o = foot + np.asarray(H)[:, None] * nn
    # NaN origins and rows past the table ride on copies of the first queries
    extra = min(8, row.size)
    o = np.concatenate([o, np.full((extra, 3), np.nan), o[:extra]])
    foot = np.concatenate([foot, foot[:extra], foot[:extra]])
    row = np.concatenate([row, row[:extra], np.array([T, T + 1, 255 + (T >= 255), 256, 1 << 16, (1 << 31) - 1, 1 << 31, (1 << 32) - 1][:extra])])
    cell = np.concatenate([np.asarray(cell, np.int64).reshape(-1, 2), np.full((2 * extra, 2), -1)])
    centre = np.concatenate([np.asarray(centre, bool), np.zeros(2 * extra, bool)])
    tag = np.asarray(tag + ["nan"] * extra + ["row_past"] * extra)
    o32 = o.astype(np.float32)
    q = dict(row=row.astype(np.uint32), o=o32, foot=foot.astype(np.float32), cell=cell, centre=centre, tag=tag)
    q["cls"] = classes(g, nuv, hmax, row, o32, T)
    return q


def image_point(g, rows, tx):
    """float64 mirror image of the points tx [n][3] in the planes of triangles `rows`"""
    n, v1 = g["n"][rows], g["v1"][rows]
    dn = ((np.asarray(tx, np.float64) - v1) * n).sum(axis=1)
    return np.asarray(tx, np.float64) - 2.0 * dn[:, None] * n


def image_variants(g, rows, o_adv, d, tx, ro_img, seed=0):
    """The mode-1 family of queries (row, o_adv, d) whose d is the mirrored direction and o_adv the advanced origin (both
    from the oracle's sequence): per query the unperturbed d, d turned about a random axis so that the line passes the
    image at IMG_FACTORS x ro_img, and d reversed.  -> dict(src [m] index of the base query, d [m][3] float32,
    kind [m], factor [m] (0 for base / reversed))."""
    rng = np.random.default_rng(seed)
    n = rows.size
    im = image_point(g, rows, tx)
    w = np.asarray(o_adv, np.float32).astype(np.float64) - im
    L = np.sqrt((w * w).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        wh = w / L[:, None]
        a = rng.normal(size=(n, 3))
        a -= (a * wh).sum(axis=1)[:, None] * wh
        a /= np.sqrt((a * a).sum(axis=1))[:, None]
        src, dd, kind, fac = [np.arange(n)], [np.asarray(d, np.float32)], [np.full(n, IMG_BASE)], [np.zeros(n)]
        for f in IMG_FACTORS:
            s = np.clip(f * float(ro_img) / L, 0.0, 1.0)
            dr = np.sqrt(1.0 - s * s)[:, None] * wh + s[:, None] * np.cross(a, wh)
            src.append(np.arange(n)); dd.append(dr.astype(np.float32)); kind.append(np.full(n, IMG_ROT)); fac.append(np.full(n, f))
        src.append(np.arange(n)); dd.append(-np.asarray(d, np.float32)); kind.append(np.full(n, IMG_REV)); fac.append(np.zeros(n))
    return dict(src=np.concatenate(src), d=np.concatenate(dd), kind=np.concatenate(kind), factor=np.concatenate(fac))


def line_distance(o, d, p):
    """float64 distance of the points p from the lines o + t d (d normalised here) and the sign of dot(o - p, d)"""
    o, d, p = (np.asarray(x, np.float64) for x in (o, d, p))
    with np.errstate(invalid="ignore", divide="ignore"):
        dh = d / np.sqrt((d * d).sum(axis=1))[:, None]
    w = o - p
    c = np.cross(w, dh)
    return np.sqrt((c * c).sum(axis=1)), (w * dh).sum(axis=1)


# ---- directions (modes 2 and 3) ----
def _face_dir(f, u, v):
    """direction of cube-map coordinates (face f = major axis + 3 (major < 0), u, v) -- csrc/hrt_kernels.hip rxt_cell:
    (u, v) = the two components that follow the major one cyclically, over the signed major one"""
    m, sgn = f % 3, (1.0 if f < 3 else -1.0)
    d = np.zeros(np.broadcast(u, v).shape + (3,))
    d[..., m] = sgn
    d[..., (m + 1) % 3] = u * sgn
    d[..., (m + 2) % 3] = v * sgn
    return d


def cell_of(d):
    """float64 restatement of rxt_cell for directions well inside a cell (the design test's use) -> (cell, margin):
    margin = distance of (u, v) from the nearest cell border in cells"""
    d = np.asarray(d, np.float64)
    a = np.abs(d)
    m = np.where((a[:, 1] > a[:, 0]) & (a[:, 1] >= a[:, 2]), 1, np.where((a[:, 2] > a[:, 0]) & (a[:, 2] > a[:, 1]), 2, 0))
    idx = np.arange(d.shape[0])
    major = d[idx, m]
    u, v = d[idx, (m + 1) % 3] / major, d[idx, (m + 2) % 3] / major
    x, y = (u * 0.5 + 0.5) * RXT_N, (v * 0.5 + 0.5) * RXT_N
    iu, iv = np.clip(np.floor(x), 0, RXT_N - 1).astype(np.int64), np.clip(np.floor(y), 0, RXT_N - 1).astype(np.int64)
    f = m + 3 * (major < 0)
    margin = np.minimum.reduce([x - iu, iu + 1 - x, y - iv, iv + 1 - y])
    return (f * RXT_N + iv) * RXT_N + iu, margin


def direction_set(n_fib=4096):
    """unit float32 directions [n][3] and their tags: the Fibonacci set; every cube-map cell's four borders +- 1 ulp
    in u and v (against every cell centre of the other coordinate); face edges and corners +- 1 ulp; the axes with
    +-0 components."""
    out, tags = [], []
    k = np.arange(n_fib) + 0.5
    z = 1.0 - 2.0 * k / n_fib
    ph = np.pi * (1.0 + np.sqrt(5.0)) * k
    s = np.sqrt(1.0 - z * z)
    out.append(np.stack([np.cos(ph) * s, np.sin(ph) * s, z], axis=1)); tags += ["fib"] * n_fib
    borders = (-1.0 + 2.0 * np.arange(RXT_N + 1) / RXT_N).astype(np.float32)
    b3 = np.concatenate([borders, np.nextafter(borders, np.float32(2)), np.nextafter(borders, np.float32(-2))]).astype(np.float64)
    centres = -1.0 + (2.0 * np.arange(RXT_N) + 1.0) / RXT_N
    B, Cc = np.meshgrid(b3, centres, indexing="ij")
    for f in range(6):
        out.append(_face_dir(f, B.reshape(-1), Cc.reshape(-1))); tags += ["border_u"] * B.size
        out.append(_face_dir(f, Cc.reshape(-1), B.reshape(-1))); tags += ["border_v"] * B.size
    one = np.float32(1.0)
    near = [1.0, float(np.nextafter(one, np.float32(2))), float(np.nextafter(one, np.float32(0)))]
    edges = []
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for p in near:
                for zc in (-0.5, 0.0, -0.0, 0.3, sx * p, -sx * p):   # |x| = |y| (+- 1 ulp) and the cube corners
                    base = np.array([sx, sy * p, zc])
                    for r in range(3):
                        edges.append(np.roll(base, r))
    out.append(np.array(edges)); tags += ["edge"] * len(edges)
    axes = []
    for r in range(3):
        for sgn in (1.0, -1.0):
            for z1 in (0.0, -0.0):
                for z2 in (0.0, -0.0):
                    axes.append(np.roll(np.array([sgn, z1, z2]), r))
    out.append(np.array(axes)); tags += ["axis"] * len(axes)
    d = np.concatenate(out)
    d = d / np.sqrt((d * d).sum(axis=1))[:, None]
    return d.astype(np.float32), np.asarray(tags)


def region_ball(tri_vtx, tx_pos):
    """float64 centre and radius of the ball every ray origin lies in (csrc/host/problem.c rxt_build): the box of the
    vertices and the TXs, its half diagonal x 1.01 + 0.01 + 1e-5 |c|_1"""
    g = geometry(tri_vtx)
    pts = np.concatenate([g["v1"], g["v1"] + g["e1"], g["v1"] + g["e2"], np.asarray(tx_pos, np.float64).reshape(-1, 3)])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    c = 0.5 * (lo + hi)
    return c, 0.5 * np.sqrt(((hi - lo) ** 2).sum()) * 1.01 + 0.01 + 1e-5 * np.abs(c).sum()


def points_on_triangles(tri_vtx, per_tri, seed=0):
    """float32 points inside every non-degenerate triangle, `per_tri` each (uniform barycentric)"""
    rng = np.random.default_rng(seed)
    g = geometry(tri_vtx)
    ok = np.flatnonzero(np.isfinite(g["n"]).all(axis=1))
    rows = np.repeat(ok, per_tri)
    a, b = rng.random(rows.size), rng.random(rows.size)
    flip = a + b > 1.0
    a, b = np.where(flip, 1.0 - a, a), np.where(flip, 1.0 - b, b)
    return rows, (g["v1"][rows] + a[:, None] * g["e1"][rows] + b[:, None] * g["e2"][rows]).astype(np.float32)


# ---- masks ----
def words_to_masks(words):
    """uint32 [n][8] mask words -> uint64 [n][4]"""
    w = np.ascontiguousarray(words, np.uint32).reshape(-1, 8)
    return w.view(np.uint64).reshape(-1, 4).copy()


def popcount(masks):
    b = np.unpackbits(np.ascontiguousarray(masks).view(np.uint8).reshape(masks.shape[0], -1), axis=1)
    return b.sum(axis=1)


def has_bit(masks, rows):
    rows = np.asarray(rows, np.int64)
    return ((masks[np.arange(masks.shape[0]), rows >> 6] >> (rows & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def clear_bit(masks, i, row):
    m = masks.copy()
    m[i, row >> 6] &= ~(np.uint64(1) << np.uint64(row & 63))
    return m


def bits_beyond(masks, num_tri):
    """queries whose mask has a bit at or beyond num_tri"""
    lim = np.zeros(masks.shape[1], np.uint64)
    for k in range(masks.shape[1]):
        nb = min(max(num_tri - 64 * k, 0), 64)
        lim[k] = np.uint64((1 << nb) - 1) if nb < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    return np.flatnonzero((masks & ~lim[None, :]).any(axis=1))


def soundness_failures(full, restricted, served, need=None):
    """indices of the served queries whose scan restricted to the lane's mask differs from the full scan in triangle or
    in distance bits (`need`: the queries the equality is asked of; default all)"""
    bad = served & ((full[0] != restricted[0]) | (full[1] != restricted[1]))
    if need is not None:
        bad &= need
    return np.flatnonzero(bad)


def describe(mode, q, i, row_of_orig, full_tri):
    """what a failure names: mode, apex, triangle and cell of the origin, the missing row"""
    win = int(full_tri[i])
    miss = int(row_of_orig[win]) if win != 0xFFFFFFFF else -1
    cell = tuple(int(x) for x in q["cell"][i]) if "cell" in q else None
    return "mode %d apex %d row %s cell (iu, iv) %s tag %s: missing row %d (flat index %d)" % (
        mode, int(q["apex"][i]), int(q["row"][i]) if "row" in q else "-", cell, q["tag"][i], miss, win)


# ---- scenes ----
GEN_RX = [[5, 3, 1.5], [-12, -8, 7], [15, 10, 10]]
GEN_TX = [[-10, 5, 6.0], [8, -9, 3]]
# appended to a generated scene (in place of its last triangles): needles whose cell coordinates cannot be rounded to
# 1 / 64 of a cell, and triangles without area -- the host refuses to serve them
BAD_TRIANGLES = np.array([
    [[0, 0, 1], [10, 0, 1], [5, 1e-3, 1]],           # needle
    [[-3, 2, 4], [-3, 12, 4.0005], [-3, 7, 4.0004]], # needle, tilted
    [[1, 1, 2], [1, 1, 2], [2, 2, 3]],               # zero area: two equal vertices (NaN normal)
    [[2, 2, 5], [4, 4, 7], [3, 3, 6]],               # zero area: collinear
], np.float32)


def generated_scene(path, n_tri, seed, tilt=False, shift=0.0, bad=False):
    """A room with clutter (tests/scenes_gen.py) of EXACTLY n_tri triangles: the last mesh loses the triangles beyond;
    `shift` translates everything by `shift` on every axis; `bad` replaces
    the last len(BAD_TRIANGLES) triangles by BAD_TRIANGLES (a mesh of their own, so they are the last flat indices).
    Returns (rx_pos, tx_pos, number of bad triangles)."""
    from oracle.oracle import read_hrt

    from . import scenes_gen as G
    n_boxes = -(-n_tri // 12) - 1 + (1 if bad else 0)
    G.room_with_clutter(str(path), max(n_boxes, 1), seed=seed, tilt=tilt, moving=False)
    meshes = read_hrt(str(path))
    keep = n_tri - (len(BAD_TRIANGLES) if bad else 0)
    out, have = [], 0
    for m in meshes:
        take = min(len(m["idx"]), keep - have)
        if take <= 0:
            break
        out.append(dict(vs=m["vs"], idx=m["idx"][:take], material_index=m["material_index"], velocity=m["velocity"]))
        have += take
    assert have == keep
    if bad:
        out.append(dict(vs=BAD_TRIANGLES.reshape(-1, 3), idx=np.arange(3 * len(BAD_TRIANGLES), dtype=np.uint32).reshape(-1, 3),
                        material_index=2, velocity=[0, 0, 0]))
    for m in out:
        m["vs"] = (np.asarray(m["vs"], np.float32) + np.float32(shift)).astype(np.float32)
    G.write_hrt(str(path), out)
    rx = (np.asarray(GEN_RX, np.float32) + np.float32(shift)).tolist()
    tx = (np.asarray(GEN_TX, np.float32) + np.float32(shift)).tolist()
    return rx, tx, (len(BAD_TRIANGLES) if bad else 0)


#: the generated tables: both ends of the patch-table range (65, 256) and the mask-word edges (128, 129)
GENERATED = dict(
    gen65_tilt=dict(n_tri=65, seed=5, tilt=True),
    gen128_far=dict(n_tri=128, seed=6, shift=300.0),
    gen129_bad=dict(n_tri=129, seed=7, bad=True),
    gen256=dict(n_tri=256, seed=8),
)
