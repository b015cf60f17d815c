"""Planted live lists for the scatter records (tests/test_gpu_records_planted.py, tests/test_records_design.py) -- numpy
plus the oracle; no GPU.

The last launch of a trace takes a live list (hit block nb - 1: per entry the origin o, already advanced 1e-4 along the
mirrored direction d, the table row it left, its incidence angle theta, four amplitudes, a delay) and writes, per
receiver IN ORDER, a scatter record (oracle/hrt_oracle.c scatter_to_receivers; src/compute_paths.c:671-723 of the
reference).  hrt_debug_last_launch runs that launch on a list the test plants; this module plants the lists.

A case = a scene, its endpoints and a MASTER list of MASTER_N states; every list the device runs is cut from it:
prefixes (LENGTHS), the master permuted (PERM), the master with every other entry replaced (replaced()).  Triangles are
FLAT (reference-order) indices here; the child maps them to table rows (hrt_problem_tri_order).

  origins     feet of candidates_util.patch_queries on the triangle's own patch grid (host_grid), mirrored off the
              triangle from a source point and advanced 1e-4 d by the oracle's own sequence (oracle.mirror);
  theta, amplitudes, tau   no two entries share a value, the four amplitudes of an entry are distinct and non-zero;
  scenes      the canyon (configs.C3 cut to 2 048 rays: 234 triangles, every one served, nothing moves) and the slab
              (scenes_gen.slab: 115 triangles, walls exactly 1 m apart, a needle no grid serves, moving meshes).

Classes (classes(): entries of the master list in the class, or waves; counts as the design test prints them):
                                                              canyon   canyon_rxperm   slab
  t_eq1     a shadow hit at t == 1.0f exactly (blocked)            0               0     12
  t_above   ... at the next float above 1 (theta overwritten)      0               0     12
  t_below   ... at the next float below 1 (blocked)                0               0     12
  carry     hit beyond 1 m at RX k, RX k + 1 clear               446             421    561
  converse  RX k clear, hit beyond 1 m at RX k + 1               141             408    464
  blocked0  blocked at RX 0, a later record unblocked            118             159    254
  f2_below  an unblocked record with f2 < 1 (no division)          0               0     12
  f2_above  an unblocked record with f2 > 1                     1130            1130    999
  f2_exact  ... with f2 == 1.0f exactly (searched, not required)   0               0      4
  served / off_grid / unserved_row   lanes by what their patch lookup does (candidates_util.classes)
                                                          1040/240/0      1040/240/0  1048/183/49
  mixed_waves          served and not-served lanes in one wave    18              18     18
  distinct_row_waves   waves on 64 different rows                  2               2      2
  moving         entries on a moving mesh                          0               0   1229
  blocker_moves  ... whose shadow hit's mesh moves differently     0               0    683

The canyon has no row without a grid and nothing that moves: the slab supplies both.  f2 == 1.0f exactly is searched for
(slab_specials) and found on the slab; dividing by exactly 1 changes nothing, so `f2 >= 1` is NOT a wrong reading (the
design test asserts that it gives the reference's bits) -- the wrong reading planted against the rule is `always
divide` (CONTROLS)."""
import numpy as np

from oracle import oracle

from . import candidates_util as CU
from . import configs as K
from . import scenes_gen as G

MASTER_N = 1280
LENGTHS = (1, 63, 64, 65, 255, 256, 257, 1023, 1025)
PERM = (np.arange(MASTER_N) * 577 + 129) % MASTER_N     # 577 is coprime to 1280: entries move across waves and chunks
POISON = 0x7FA5A5A5                                      # a NaN whose bytes are mostly 0xA5; bits 0x100 (a void step) set
NO_HIT = oracle.NO_HIT
ONE = np.float32(1.0)
T_EQ1 = int(ONE.view(np.uint32))
T_ABOVE = int(np.nextafter(ONE, np.float32(2)).view(np.uint32))
T_BELOW = int(np.nextafter(ONE, np.float32(0)).view(np.uint32))
FIELDS = oracle.REC_FIELDS
CASES = ("canyon", "canyon_rxperm", "slab")
RX_PERM = (2, 0, 3, 1)


def host_hmax(flat):
    """hrt_kpatch.hmax as csrc/host/problem.c patch_build forms it: 4e-4 + 4e-6 * sum_k max(|lo_k|, |hi_k|) of the
    float32 box of the vertices"""
    v = flat["tri_vtx"].reshape(-1, 3)
    v = v[np.isfinite(v).all(axis=1)]
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    return np.float32(4e-4 + 4e-6 * np.maximum(np.abs(lo), np.abs(hi)).sum())


def table(scene_path):
    flat = oracle.flatten(oracle.read_hrt(scene_path))
    return dict(path=str(scene_path), flat=flat, T=flat["tri_vtx"].shape[0], g=CU.geometry(flat["tri_vtx"]),
                nuv=CU.host_grid(flat["tri_vtx"]), hmax=host_hmax(flat))


def scene(name, tmp_dir):
    """-> dict(scene_path, rx_pos, tx_pos, f_ghz, num_paths) of a case; the slab is written into tmp_dir"""
    if name.startswith("canyon"):
        c = K.small(K.C3, 2048)
        rx = c["rx_pos"] if name == "canyon" else [c["rx_pos"][k] for k in RX_PERM]
        return dict(scene_path=c["scene_path"], rx_pos=rx, tx_pos=c["tx_pos"], f_ghz=c["f_ghz"], num_paths=2048)
    import os
    path = os.path.join(str(tmp_dir), "slab.hrt")
    G.slab(path, moving=True)
    return dict(scene_path=path, rx_pos=G.SLAB_RX, tx_pos=G.SLAB_TX, f_ghz=3.5, num_paths=2048)


# ---- states ----
def _advance(tb, tri, src, foot):
    """the oracle's bounce: d = the direction src -> foot mirrored off triangle tri, o = foot + 1e-4 d"""
    return oracle.mirror(tb["flat"], tri, src, foot, foot)


def pool(tb, sources, seed=3):
    """every distinct foot of candidates_util.patch_queries (flat order), mirrored from sources[i % len]:
    dict(tri, o, d, cls (candidates_util.classes of the ADVANCED origin), tag)"""
    q = CU.patch_queries(tb["flat"]["tri_vtx"], tb["nuv"], tb["hmax"], seed=seed, spread=1)
    keep = (q["row"] < tb["T"]) & np.isfinite(q["foot"]).all(axis=1) & (q["tag"] != "nan")
    key = np.concatenate([q["row"][:, None].astype(np.uint32), q["foot"].view(np.uint32)], axis=1)
    _, first = np.unique(key, axis=0, return_index=True)
    sel = np.sort(first[keep[first]])
    tri, foot, tag = q["row"][sel].astype(np.uint32), q["foot"][sel], q["tag"][sel]
    src = np.asarray(sources, np.float32).reshape(-1, 3)[np.arange(sel.size) % len(sources)]
    d, o = _advance(tb, tri, src, foot)
    ok = np.isfinite(d).all(axis=1) & np.isfinite(o).all(axis=1)
    tri, o, d, tag = tri[ok], o[ok], d[ok], tag[ok]
    return dict(tri=tri, o=o, d=d, tag=tag, cls=CU.classes(tb["g"], tb["nuv"], tb["hmax"], tri, o, tb["T"]))


def shadows(tb, rx_pos, o):
    """the oracle's shadow scan of every (rx, origin): tri [nrx][n] (NO_HIT: clear), t bits [nrx][n]"""
    rx = np.asarray(rx_pos, np.float32).reshape(-1, 3)
    tri, t = [], []
    for k in range(rx.shape[0]):
        w = oracle.shadow_dirs(o, np.tile(rx[k], (o.shape[0], 1)))
        a, b = oracle.closest_hits(tb["flat"], o, w)
        tri.append(a); t.append(b)
    return np.stack(tri), np.stack(t)


def f2_of(f_ghz, rx, o):
    """f2 = (fsl_mult |rx - o|)^2 in the reference's float sequence (src/compute_paths.c:483-488, :711-713)"""
    f_hz = np.float32(np.float64(np.float32(f_ghz)) * 1e9)
    fsl = np.float32(4.0) * np.float32(3.14159265358979323846) * f_hz / np.float32(299792458.0)
    w = (np.asarray(rx, np.float32) - np.asarray(o, np.float32)).astype(np.float32)
    d2 = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
    f2 = fsl * d2
    return f2 * f2


def slab_specials(tb, f_ghz):
    """States of the slab that need a float coincidence, found by SEARCH over the foot's x coordinate (steps of 2^-26
    around the value that would put the advanced origin where the coincidence lies), keeping what the oracle reports:
    shadow hits on wall B at t == 1, the next float above and the next below, from wall A towards RX 1; origins on
    wall A with f2 of RX 2 below 1, above 1 and, if found, exactly 1.  -> dict(tri, o, d, want [n] str)"""
    rx = np.asarray(G.SLAB_RX, np.float32)
    step = 2.0 ** -26
    tri_l, o_l, d_l, want_l = [], [], [], []
    wall_a = 2    # flat index of wall A's first triangle (v1 = (0, -2, 0), e1 = (0, 4, 0), e2 = (0, 4, 4): y >= z - 2 ... )
    srcs = np.array([[0.5, -3.0, 1.5], [0.75, 1.5, 3.5], [0.25, 0.0, 0.5], [0.5, 1.0, 0.25]], np.float32)
    # ---- t == 1 and its neighbours: feet at lateral distance r from RX 1's foot (0, 0.5, 2) on wall A ----
    for r, ang in ((0.0, 0.0), (0.02, 0.3), (0.04, 2.0), (0.06, 4.0)):
        for s in srcs[:3]:
            y, z = 0.5 + r * np.cos(ang), 2.0 + r * np.sin(ang)
            d0, _ = _advance(tb, [wall_a], [s], [[0.0, y, z]])
            x0 = r * r / 18.0 - 1e-4 * float(d0[0, 0])
            fx = (x0 + step * np.arange(-96, 97)).astype(np.float32)
            foot = np.stack([fx, np.full(fx.size, y, np.float32), np.full(fx.size, z, np.float32)], axis=1)
            d, o = _advance(tb, np.full(fx.size, wall_a, np.uint32), np.tile(s, (fx.size, 1)), foot)
            w = oracle.shadow_dirs(o, np.tile(rx[1], (fx.size, 1)))
            _, t = oracle.closest_hits(tb["flat"], o, w)
            for name, bits in (("t_eq1", T_EQ1), ("t_above", T_ABOVE), ("t_below", T_BELOW)):
                hit = np.flatnonzero(t == bits)
                if hit.size:
                    k = hit[hit.size // 2]
                    tri_l.append(wall_a); o_l.append(o[k]); d_l.append(d[k]); want_l.append(name)
    # ---- f2 of RX 2 (2^-8 m in front of wall A at y = 0.25, z = 1.25): the rule flips at |rx - o| = 1 / fsl_mult ----
    f_hz = np.float32(np.float64(np.float32(f_ghz)) * 1e9)
    r1 = 1.0 / float(np.float32(4.0) * np.float32(3.14159265358979323846) * f_hz / np.float32(299792458.0))
    for k, s in enumerate(srcs):
        for frac in (0.0, 0.5, 0.9, 1.0, 1.1, 1.5):
            # lateral distance that puts the advanced origin at frac * r1 from the RX (frac = 0: straight in front)
            hx = float(rx[2, 0]) - 1e-4
            lat = np.sqrt(max((frac * r1) ** 2 - hx * hx, 0.0))
            y, z = 0.25 + lat * np.cos(1.0 + k), 1.25 + lat * np.sin(1.0 + k)
            if frac == 1.0:   # the search for f2 == 1.0f exactly: move the foot along x until |rx - o| = r1, then scan
                fc = 0.0
                for _ in range(4):
                    _, oc = _advance(tb, [wall_a], [s], [[fc, y, z]])
                    wv = rx[2].astype(np.float64) - oc[0].astype(np.float64)
                    dist = np.sqrt((wv * wv).sum())
                    fc += (dist - r1) * dist / wv[0]
                fx = (fc + step * np.arange(-4096, 4097) / 64.0).astype(np.float32)
            else:
                fx = np.zeros(1, np.float32)
            foot = np.stack([fx, np.full(fx.size, y, np.float32), np.full(fx.size, z, np.float32)], axis=1)
            d, o = _advance(tb, np.full(fx.size, wall_a, np.uint32), np.tile(s, (fx.size, 1)), foot)
            f2 = f2_of(f_ghz, rx[2], o)
            pick = np.flatnonzero(f2 == ONE) if frac == 1.0 else np.arange(1)
            if pick.size:
                j = pick[pick.size // 2]
                tri_l.append(wall_a); o_l.append(o[j]); d_l.append(d[j])
                want_l.append("f2_exact" if frac == 1.0 else ("f2_below" if f2[j] < ONE else "f2_above"))
    return dict(tri=np.asarray(tri_l, np.uint32), o=np.asarray(o_l, np.float32).reshape(-1, 3),
                d=np.asarray(d_l, np.float32).reshape(-1, 3), want=np.asarray(want_l))


def _values(n):
    """theta, amplitudes, tau of n entries: no two entries share a value; an entry's amplitudes are distinct, non-zero"""
    u = (np.arange(n, dtype=np.float64) + 1.0) / (n + 1.0)
    theta = (0.03 + 1.5 * u).astype(np.float32)
    amp = np.stack([0.9 - 0.4 * u, 0.21 + 0.25 * u, -0.7 + 0.45 * u, 0.05 + 0.13 * u], axis=1).astype(np.float32)
    tau = (1e-8 * (1.0 + 7.0 * u)).astype(np.float32)
    return theta, amp, tau


_cache = {}


def case(name, tmp_dir):
    """-> dict(scene (scene()), tb (table()), states (the master list: tri, o, d, theta, amp, tau), cls, tag)"""
    if name in _cache:
        return _cache[name]
    sc = scene(name, tmp_dir)
    tb = table(sc["scene_path"])
    tx = np.asarray(sc["tx_pos"], np.float32).reshape(-1, 3)
    if name == "slab":
        sources = np.concatenate([tx, [[0.75, 1.5, 3.5], [6.0, -2.0, 3.0], [-1.0, -4.0, 2.0], [4.0, 3.0, 5.0]]]).astype(np.float32)
    else:
        sources = np.concatenate([tx, [[0.0, 0.0, 6.0], [20.0, 1.0, 2.0], [-20.0, -2.0, 1.0]]]).astype(np.float32)
    P = pool(tb, sources)
    rng = np.random.default_rng(17)
    served = np.flatnonzero(P["cls"] == CU.MUST)
    off = np.flatnonzero((P["cls"] == CU.MUST_NOT) & (P["tag"] == "outside") & (tb["nuv"][P["tri"], 0] > 0))
    unrow = np.flatnonzero(tb["nuv"][P["tri"], 0] == 0)
    order = []
    # two waves on 64 different rows each
    by_row = {}
    for i in served:
        by_row.setdefault(int(P["tri"][i]), []).append(int(i))
    rows = sorted(by_row)
    assert len(rows) >= 64
    for w in range(2):
        pick = [rows[(w * 37 + k * (len(rows) // 64)) % len(rows)] for k in range(64)]
        assert len(set(pick)) == 64
        order += [by_row[r][w % len(by_row[r])] for r in pick]
    # six mixed waves: served lanes, lanes off their row's grid, lanes on a row without a grid, shuffled inside the wave
    for w in range(6):
        n_un = 8 if unrow.size else 0
        lanes = np.concatenate([rng.choice(served, 40, replace=False), rng.choice(off, 24 - n_un, replace=False),
                                rng.choice(unrow, n_un, replace=True) if n_un else np.zeros(0, np.int64)])
        order += list(rng.permutation(lanes))
    base = dict(tri=P["tri"][order], o=P["o"][order], d=P["d"][order])
    cls, tag = list(P["cls"][order]), list(P["tag"][order])
    if name == "slab":   # the searched states, spread over the list by the fill below
        S = slab_specials(tb, sc["f_ghz"])
        for k in ("tri", "o", "d"):
            base[k] = np.concatenate([base[k], S[k]])
        cls += list(CU.classes(tb["g"], tb["nuv"], tb["hmax"], S["tri"], S["o"], tb["T"]))
        tag += list(S["want"])
    n_fill = MASTER_N - len(tag)
    assert n_fill > 0
    unserved = np.concatenate([off, unrow])
    fill = np.concatenate([rng.choice(served, n_fill - n_fill // 8, replace=n_fill > served.size),
                           rng.choice(unserved, n_fill // 8, replace=True)])
    fill = rng.permutation(fill)
    for k in ("tri", "o", "d"):
        base[k] = np.concatenate([base[k], P[k][fill]])
    cls += list(P["cls"][fill]); tag += list(P["tag"][fill])
    # the first 512 entries keep their waves; the rest (specials and fill) is shuffled together
    tail = 512 + rng.permutation(MASTER_N - 512)
    idx = np.concatenate([np.arange(512), tail])
    states = {k: np.ascontiguousarray(v[idx]) for k, v in base.items()}
    states["theta"], states["amp"], states["tau"] = _values(MASTER_N)
    out = dict(name=name, scene=sc, tb=tb, states=states, cls=np.asarray(cls)[idx], tag=np.asarray(tag)[idx])
    _cache[name] = out
    return out


def take(states, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in states.items()}


def replaced(states):
    """the master list with every other entry (the odd ones) replaced by a different valid state"""
    n = states["tri"].shape[0]
    src = np.where(np.arange(n) % 2 == 1, (np.arange(n) + 641) % n, np.arange(n))
    src = np.where((np.arange(n) % 2 == 1) & (src % 2 == 1), (src + 1) % n, src)   # (from an even slot: never itself)
    return take(states, src)


def lists(c):
    """every list the device runs for a case, name -> indices into the master list (a list = take(master, idx));
    `replaced` is given by replaced()"""
    out = {"n%d" % n: np.arange(n) for n in LENGTHS}
    out["perm"] = PERM
    return out


def reference(c, states=None):
    st = c["states"] if states is None else states
    return oracle.scatter_records(c["tb"]["flat"], c["scene"]["f_ghz"], c["scene"]["rx_pos"], st)


# ---- classes ----
def classes(c):
    """name -> indices of the master list (per entry) in that class, from the oracle alone"""
    st, tb, sc = c["states"], c["tb"], c["scene"]
    rx = np.asarray(sc["rx_pos"], np.float32)
    tri, t = shadows(tb, rx, st["o"])
    hit = tri != NO_HIT
    tf = t.view(np.float32)
    far = hit & (tf > ONE)
    ref = reference(c)
    ub = ref["unblocked"]
    f2 = np.stack([f2_of(sc["f_ghz"], rx[k], st["o"]) for k in range(rx.shape[0])])
    mesh = tb["flat"]["tri_mesh"][st["tri"]]
    moving = np.abs(tb["flat"]["mesh_velocity"][mesh]).sum(axis=1) > 0
    served = c["cls"] == CU.MUST
    unrow = tb["nuv"][st["tri"], 0] == 0
    notserved = (c["cls"] == CU.MUST_NOT)
    n = st["tri"].shape[0]
    waves = np.arange(n) // 64
    mixed = [w for w in range(n // 64) if served[waves == w].any() and notserved[waves == w].any()]
    distinct = [w for w in range(n // 64) if np.unique(st["tri"][waves == w]).size == 64]
    anyrx = lambda m: np.flatnonzero(m.any(axis=0))   # noqa: E731
    out = dict(
        t_eq1=anyrx(hit & (t == T_EQ1)), t_above=anyrx(hit & (t == T_ABOVE)), t_below=anyrx(hit & (t == T_BELOW)),
        carry=anyrx(far[:-1] & ~hit[1:]), converse=anyrx(~hit[:-1] & far[1:]),
        blocked0=np.flatnonzero(~ub[0] & ub[1:].any(axis=0)),
        f2_below=anyrx(ub & (f2 < ONE)), f2_above=anyrx(ub & (f2 > ONE)), f2_exact=anyrx(ub & (f2 == ONE)),
        served=np.flatnonzero(served), off_grid=np.flatnonzero(notserved & ~unrow), unserved_row=np.flatnonzero(unrow),
        mixed_waves=np.asarray(mixed), distinct_row_waves=np.asarray(distinct),
        moving=np.flatnonzero(moving), blocker_moves=anyrx(far & ub & _blocker_differs(tb, st, tri)),
    )
    out["_shadow"] = (tri, t)
    out["_ref"] = ref
    out["_f2"] = f2
    return out


def _blocker_differs(tb, st, sh_tri):
    """[nrx][n]: the shadow hit's mesh moves differently from the entry's"""
    fm, mv = tb["flat"]["tri_mesh"], tb["flat"]["mesh_velocity"]
    own = mv[fm[st["tri"]]]
    blk = mv[fm[np.where(sh_tri == NO_HIT, 0, sh_tri)]]
    return (sh_tri != NO_HIT) & (own[None] != blk).any(axis=2)


# ---- wrong readings the cases catch ----
def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _dop(f_ghz):
    f_hz = np.float32(np.float64(np.float32(f_ghz)) * 1e9)
    return f_hz / np.float32(299792458.0)


def _w_of(ref):
    """the shadow direction back from a record's arrival direction (-w): [nrx][n][3]"""
    return -np.stack([ref["dirx"], ref["diry"], ref["dirz"]], axis=2)


def dfs_numpy(c, ref, sign=-1.0, mvel=None):
    """dot(w -+ d, mvel) * dop_mult in the reference's float sequence; mvel [nrx][n][3] or None: the entry's own mesh"""
    st, tb = c["states"], c["tb"]
    if mvel is None:
        mvel = tb["flat"]["mesh_velocity"][tb["flat"]["tri_mesh"][st["tri"]]][None]
    w = _w_of(ref)
    v = (w - st["d"][None]) if sign < 0 else (w + st["d"][None])
    return (_dot3(v.astype(np.float32), np.asarray(mvel, np.float32)) * _dop(c["scene"]["f_ghz"])).astype(np.float32)


def _single_rx(c, theta_in):
    """every receiver ALONE (no carry from the others), entry i of receiver k starting from theta_in[k][i]"""
    rx = np.asarray(c["scene"]["rx_pos"], np.float32)
    outs = []
    for k in range(rx.shape[0]):
        st = dict(c["states"]); st["theta"] = np.ascontiguousarray(theta_in[k], np.float32)
        outs.append(oracle.scatter_records(c["tb"]["flat"], c["scene"]["f_ghz"], rx[k:k + 1], st))
    return {f: np.concatenate([o[f] for o in outs]) for f in outs[0]}


def control(c, name, cl):
    """the records a WRONG reading of the rule gives for the master list of case c (cl = classes(c)); every one must
    differ from the reference somewhere (tests/test_records_design.py).  Built from the oracle's own outputs: the loop
    run with changed inputs, or float32 numpy on its per-receiver results."""
    st, tb, sc = c["states"], c["tb"], c["scene"]
    ref = cl["_ref"]
    out = {k: v.copy() for k, v in ref.items()}
    sh_tri, t = cl["_shadow"]
    hit = sh_tri != NO_HIT
    nrx = hit.shape[0]
    if name == "blocked_at_t_lt_1":       # `t < 1`: a hit at exactly one metre no longer blocks
        out["unblocked"] = ref["unblocked"] | (hit & (t == T_EQ1))
    elif name == "theta_not_carried":     # every receiver starts from the entry's own theta
        out = _single_rx(c, np.tile(st["theta"], (nrx, 1)))
    elif name == "theta_from_blocking_hits_only":
        # a hit beyond one metre does not overwrite theta: receivers WITHOUT a hit start from the last BLOCKING hit's
        # angle (else the entry's own); receivers with a hit keep the reference's record (not expressible here)
        th_hit = _hit_theta(c, sh_tri)
        blocking = hit & (t.view(np.float32) <= ONE)
        th = np.tile(st["theta"], (nrx, 1))
        cur = st["theta"].copy()
        for k in range(nrx):
            th[k] = cur
            cur = np.where(blocking[k], th_hit[k], cur)
        alone = _single_rx(c, th)
        for f in out:
            out[f] = np.where(hit, ref[f], alone[f])
    elif name == "f2_ge_1":               # `f2 >= 1`: divides by exactly 1 where f2 == 1 -- the same bits (module text)
        f2 = cl["_f2"]
        m = ref["unblocked"] & (f2 == ONE)
        for f in ("a_te_re", "a_te_im", "a_tm_re", "a_tm_im"):
            out[f] = np.where(m, (ref[f] / f2).astype(np.float32), ref[f])
    elif name == "always_divide":         # no threshold: the amplitudes of f2 < 1 records are divided too
        f2 = cl["_f2"]
        m = ref["unblocked"] & (f2 < ONE)
        for f in ("a_te_re", "a_te_im", "a_tm_re", "a_tm_im"):
            out[f] = np.where(m, (ref[f] / f2).astype(np.float32), ref[f])
    elif name == "rx_order_reversed":
        rx = np.asarray(sc["rx_pos"], np.float32)[::-1]
        r = oracle.scatter_records(tb["flat"], sc["f_ghz"], rx, st)
        out = {k: v[::-1].copy() for k, v in r.items()}
    elif name == "dfs_from_w_plus_d":
        out["dfs"] = np.where(ref["unblocked"], dfs_numpy(c, ref, +1.0), ref["dfs"])
    elif name == "mvel_of_the_blocker":   # the velocity of the shadow hit's mesh where there is one
        fm, mv = tb["flat"]["tri_mesh"], tb["flat"]["mesh_velocity"]
        own = mv[fm[st["tri"]]]
        mvel = np.where(hit[..., None], mv[fm[np.where(hit, sh_tri, 0)]], own[None])
        out["dfs"] = np.where(ref["unblocked"], dfs_numpy(c, ref, -1.0, mvel), ref["dfs"])
    elif name == "te_tm_swapped":
        s2 = dict(st); s2["amp"] = np.ascontiguousarray(st["amp"][:, [2, 3, 0, 1]])
        out = reference(c, s2)
    elif name == "tau_without_own":
        s2 = dict(st); s2["tau"] = np.zeros_like(st["tau"])
        out = reference(c, s2)
    else:
        raise KeyError(name)
    return out


CONTROLS = ("blocked_at_t_lt_1", "theta_not_carried", "theta_from_blocking_hits_only", "always_divide",
            "rx_order_reversed", "dfs_from_w_plus_d", "mvel_of_the_blocker", "te_tm_swapped", "tau_without_own")


def _hit_theta(c, sh_tri):
    """the incidence angle of every shadow hit [nrx][n] (0 where there is none): the reference's formula
    (src/compute_paths.c:281-283) through the host libm, on the shadow direction the oracle forms"""
    tb, st = c["tb"], c["states"]
    rx = np.asarray(c["scene"]["rx_pos"], np.float32)
    n = tb["g"]["n"].astype(np.float32)   # (the float32 normals: exact for the axis-aligned walls the control needs)
    out = np.zeros(sh_tri.shape, np.float32)
    for k in range(rx.shape[0]):
        w = oracle.shadow_dirs(st["o"], np.tile(rx[k], (st["o"].shape[0], 1)))
        nn = n[np.where(sh_tri[k] == NO_HIT, 0, sh_tri[k])]
        out[k] = oracle.host_libm("incidence_angle", _dot3(nn, w).astype(np.float32))
    return out


def differs(a, b, n=None):
    """number of (rx, entry) slots in which two record sets differ in any field's bits or in the unblocked flag"""
    bad = a["unblocked"] != b["unblocked"]
    for f in FIELDS:
        bad |= np.ascontiguousarray(a[f]).view(np.uint32) != np.ascontiguousarray(b[f]).view(np.uint32)
    return int(bad[:, :n].sum())
