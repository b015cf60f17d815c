"""The pure-numpy parts of tests/candidates_util.py (no GPU): the planted queries are what the design promises -- every
query lies in the class it claims (checked in float64 by an independent formulation), every class is non-empty on
every test scene, the mode-1 lines pass the image where they are meant to, the direction set reaches every cube-map
cell and its borders -- the host's serving rule serves the whole canyon, and the soundness check reports exactly the
query whose mask lost its winner."""
import os

import numpy as np
import pytest

from oracle import oracle

from . import candidates_util as CU
from . import configs as K

SCENES = ["canyon"] + list(CU.GENERATED)


def host_margins(tri_vtx, rx, tx):
    """hmax and ro_img as csrc/host/problem.c patch_build forms them (float32)"""
    g = CU.geometry(tri_vtx)
    pts = np.concatenate([g["v1"], g["v1"] + g["e1"], g["v1"] + g["e2"]])
    pts = pts[np.isfinite(pts).all(axis=1)]
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    ext1 = (hi - lo).sum()
    cmax = np.maximum(np.abs(lo), np.abs(hi)).sum()
    hmax = np.float32(4e-4 + 4e-6 * cmax)
    for a in np.concatenate([np.asarray(rx, np.float64), np.asarray(tx, np.float64)]):
        cmax = max(cmax, np.abs(a).sum())
    return hmax, np.float32(1e-3 + 1e-5 * (cmax + ext1))


@pytest.fixture(scope="module", params=SCENES)
def scene(request, tmp_path_factory):
    name = request.param
    if name == "canyon":
        c = K.IN_PLANE["canyon"]
        path, rx, tx, n_bad = c["scene_path"], c["rx_pos"], c["tx_pos"], 0
    else:
        path = os.path.join(str(tmp_path_factory.mktemp("cand_design")), name + ".hrt")
        rx, tx, n_bad = CU.generated_scene(path, **CU.GENERATED[name])
    flat = oracle.flatten(oracle.read_hrt(path))
    vtx = flat["tri_vtx"]
    nuv = CU.host_grid(vtx)
    hmax, ro_img = host_margins(vtx, rx, tx)
    q = CU.patch_queries(vtx, nuv, hmax, seed=11)
    return dict(name=name, flat=flat, vtx=vtx, nuv=nuv, hmax=hmax, ro_img=ro_img, q=q, rx=np.asarray(rx, np.float32),
                tx=np.asarray(tx, np.float32), n_bad=n_bad)


def true_coordinates(vtx, nuv, rows, o):
    """(fu, fv, h) by least squares on [e1 e2 n] x = o - v1: another route than the dual basis of candidates_util"""
    t = np.asarray(vtx, np.float32).reshape(-1, 3, 3)
    out = np.full((len(rows), 3), np.nan)
    for i, (j, p) in enumerate(zip(rows, np.asarray(o, np.float32).astype(np.float64))):
        e1 = (t[j, 1] - t[j, 0]).astype(np.float64)
        e2 = (t[j, 2] - t[j, 0]).astype(np.float64)
        n = np.cross(e1, e2)
        if not np.isfinite(p).all() or not n.any():
            continue
        n /= np.linalg.norm(n)
        x = np.linalg.lstsq(np.stack([e1, e2, n], axis=1), p - t[j, 0].astype(np.float64), rcond=None)[0]
        out[i] = x[0] * nuv[j, 0], x[1] * nuv[j, 1], x[2]
    return out


def test_scenes_are_what_the_test_asks_for(scene):
    T = scene["vtx"].shape[0]
    nuv = scene["nuv"]
    if scene["name"] == "canyon":
        # 234 triangles, every one served by the host's rule at the default patch edge
        assert T == 234 and (nuv[:, 0] > 0).all()
        g = CU.geometry(scene["vtx"])
        in_plane = 0   # the endpoints lie in planes of triangles (to the rounding of a normal): the reference's noise regime
        for r in np.concatenate([scene["rx"], scene["tx"]]):
            h = ((r.astype(np.float64) - g["v1"]) * g["n"]).sum(axis=1)
            in_plane += int(np.abs(h).min() < 1e-5)
        assert in_plane >= 4 and len(scene["rx"]) == 4 and len(scene["tx"]) == 2
    else:
        assert T == CU.GENERATED[scene["name"]]["n_tri"] and 64 < T <= CU.PATCH_MAX_TRI
        assert (nuv[:T - scene["n_bad"], 0] > 0).all()
        assert not nuv[T - scene["n_bad"]:].any()   # needles and triangles without area: refused
    if scene["name"] == "gen128_far":
        assert np.abs(scene["vtx"]).min() > 250.0
    if scene["name"] == "gen65_tilt":
        n = CU.geometry(scene["vtx"])["n"]
        assert (np.abs(n).max(axis=1) < 0.999).sum() > 30   # normals off the axes


def test_every_query_is_in_the_class_it_claims(scene):
    q, nuv, T, hmax = scene["q"], scene["nuv"].astype(np.float64), scene["vtx"].shape[0], float(scene["hmax"])
    rows, cls = q["row"].astype(np.int64), q["cls"]
    rng = np.random.default_rng(4)
    pick = np.concatenate([np.flatnonzero(q["tag"] != "border_uv"), rng.choice(np.flatnonzero(q["tag"] == "border_uv"), 2000)])
    pick = pick[rng.permutation(pick.size)[:12000]]
    pick = np.concatenate([pick, np.flatnonzero(np.isin(q["tag"], ("nan", "row_past", "unserved", "outside")))])
    in_tab = rows[pick] < T
    x = true_coordinates(scene["vtx"], nuv, np.where(in_tab, rows[pick], 0), q["o"][pick])
    nu, nv = nuv[np.where(in_tab, rows[pick], 0)].T
    with np.errstate(invalid="ignore"):
        out_by = np.maximum.reduce([-x[:, 0], x[:, 0] - nu, -x[:, 1], x[:, 1] - nv])
        ok_tri = in_tab & (nu > 0) & np.isfinite(x).all(axis=1)
        must = ok_tri & (out_by <= 1.0 / 64 + 1e-9) & (np.abs(x[:, 2]) <= hmax - 1e-5 + 1e-12)
        never = ~ok_tri | (out_by > CU.PATCH_ACCEPT + 1.0 / 64 - 1e-9) | (np.abs(x[:, 2]) >= hmax * (1 + 2.0 ** -7) - 1e-12)
    c = cls[pick]
    assert must[c == CU.MUST].all() and never[c == CU.MUST_NOT].all()
    assert not (must & never).any()
    # what the tags promise
    tag = q["tag"][pick]
    assert (c[np.isin(tag, ("nan", "row_past", "unserved"))] == CU.MUST_NOT).all()
    assert (cls[q["centre"]] == CU.MUST).all() and q["centre"].sum() >= (nuv[:, 0] > 0).sum()
    for k in (CU.MUST, CU.EITHER, CU.MUST_NOT):
        assert (cls == k).sum() > 0, "class %d is empty on %s" % (k, scene["name"])
    out = q["tag"] == "outside"
    assert {CU.MUST, CU.EITHER, CU.MUST_NOT} <= set(cls[out])   # the strip: served, either, refused
    # each served triangle: its four corner cells, its last cell, a centre at every height, both NaN and rows past
    for j in np.flatnonzero(nuv[:, 0] > 0)[:: max(1, T // 40)]:
        cells = {tuple(cc) for cc in q["cell"][(rows == j) & q["centre"]]}
        nu_j, nv_j = int(nuv[j, 0]), int(nuv[j, 1])
        assert {(0, 0), (nu_j - 1, 0), (0, nv_j - 1), (nu_j - 1, nv_j - 1)} <= cells
    assert (q["tag"] == "nan").sum() > 0 and np.isnan(q["o"][q["tag"] == "nan"]).all()
    assert (q["row"][q["tag"] == "row_past"] >= T).all()
    # the half of the parallelogram beyond the triangle is planted too
    fu, fv, _ = CU.cell_coords(CU.geometry(scene["vtx"]), np.where(rows < T, rows, 0), scene["nuv"], q["o"])
    with np.errstate(invalid="ignore"):
        beyond = (cls == CU.MUST) & (fu / np.maximum(nuv[np.where(rows < T, rows, 0), 0], 1) + fv / np.maximum(nuv[np.where(rows < T, rows, 0), 1], 1) > 1.2)
    assert beyond.sum() > 0


def test_image_lines_pass_where_they_are_meant_to(scene):
    q, T = scene["q"], scene["vtx"].shape[0]
    g = CU.geometry(scene["vtx"])
    sel = np.flatnonzero((q["cls"] == CU.MUST) & (q["row"] < T))[::7]
    rows = q["row"][sel].astype(np.int64)
    tx = scene["tx"][np.arange(sel.size) % scene["tx"].shape[0]]
    d0, o_adv = oracle.mirror(scene["flat"], rows, tx, q["foot"][sel], q["o"][sel])
    var = CU.image_variants(g, rows, o_adv, d0, tx, scene["ro_img"], seed=3)
    im = CU.image_point(g, rows, tx)[var["src"]]
    dist, along = CU.line_distance(o_adv[var["src"]], var["d"], im)
    ro, hmax = float(scene["ro_img"]), float(scene["hmax"])
    base, rev = var["kind"] == CU.IMG_BASE, var["kind"] == CU.IMG_REV
    assert hmax < 0.5 * ro   # a served origin's own line passes well inside the image ball
    assert (dist[base] <= hmax + 2e-5).all() and (along[base] > 0).all()
    assert (along[rev] < 0).all()
    for f in CU.IMG_FACTORS:
        k = (var["kind"] == CU.IMG_ROT) & (var["factor"] == f)
        assert k.sum() == sel.size and (np.abs(dist[k] / ro - f) < 0.02).all() and (along[k] > 0).all(), f
    n = np.sqrt((var["d"].astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(n - 1.0).max() < 1e-6


def test_direction_set_reaches_every_cell_and_border():
    d, tag = CU.direction_set()
    assert d.dtype == np.float32 and np.abs(np.sqrt((d.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() < 1e-6
    cell, margin = CU.cell_of(d)
    assert set(np.unique(cell)) == set(range(6 * CU.RXT_N * CU.RXT_N))
    for t in ("border_u", "border_v"):
        assert (margin[tag == t] < 1e-5).all()
    assert (margin[tag == "fib"] > 1e-4).sum() > 3000
    a = np.abs(d[tag == "edge"].astype(np.float64))
    a.sort(axis=1)
    assert (np.abs(a[:, 2] - a[:, 1]) < 2e-7).all()        # two components of (nearly) equal size
    assert (np.abs(a[:, 1] - a[:, 0]) < 2e-7).sum() >= 8   # the cube corners
    ax = d[tag == "axis"]
    assert ((ax != 0).sum(axis=1) == 1).all() and np.signbit(ax).any() and len(ax) == 24
    # both signs of zero next to every axis
    assert {(bool(np.signbit(v[1])), bool(np.signbit(v[2]))) for v in ax[:4]} == {(False, False), (False, True), (True, False), (True, True)}


def test_region_ball_and_points():
    c = K.C4
    flat = oracle.flatten(oracle.read_hrt(c["scene_path"]))
    assert flat["tri_vtx"].shape[0] <= 64
    ctr, R = CU.region_ball(flat["tri_vtx"], c["tx_pos"])
    rows, pts = CU.points_on_triangles(flat["tri_vtx"], 16)
    assert (np.sqrt(((pts - ctr) ** 2).sum(axis=1)) < R).all()
    assert (np.sqrt(((np.asarray(c["tx_pos"]) - ctr) ** 2).sum(axis=1)) < R).all()
    g = CU.geometry(flat["tri_vtx"])
    h = ((pts.astype(np.float64) - g["v1"][rows]) * g["n"][rows]).sum(axis=1)
    assert np.abs(h).max() < 1e-5


def test_soundness_check_reports_exactly_the_changed_query():
    rng = np.random.default_rng(5)
    n, T = 500, 200
    tri = rng.integers(0, T, n).astype(np.uint32)
    tri[::9] = 0xFFFFFFFF
    dist = rng.integers(1, 2 ** 30, n).astype(np.uint32)
    served = rng.random(n) < 0.8
    full = (tri, dist)
    assert CU.soundness_failures(full, (tri.copy(), dist.copy()), served).size == 0
    k = int(np.flatnonzero(served)[17])
    t2, d2 = tri.copy(), dist.copy()
    t2[k] = (t2[k] + 1) % T
    assert CU.soundness_failures(full, (t2, dist), served).tolist() == [k]
    d2[k] += 1   # the same triangle at another distance is a failure too
    assert CU.soundness_failures(full, (tri, d2), served).tolist() == [k]
    u = int(np.flatnonzero(~served)[3])
    t3 = tri.copy()
    t3[u] = 0xFFFFFFFF if t3[u] != 0xFFFFFFFF else 1
    assert CU.soundness_failures(full, (t3, dist), served).size == 0   # an unserved lane walks the whole table
    # the mask helpers
    words = rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    m = CU.words_to_masks(words)
    assert m.shape == (n, 4) and int(m[3, 1]) == int(words[3, 2]) | (int(words[3, 3]) << 32)
    assert CU.popcount(m)[5] == sum(bin(int(w)).count("1") for w in words[5])
    rows = rng.integers(0, 256, n)
    bit = CU.has_bit(m, rows)
    assert bit[7] == bool((int(words[7, rows[7] >> 5]) >> (rows[7] & 31)) & 1)
    i = int(np.flatnonzero(bit)[0])
    c = CU.clear_bit(m, i, int(rows[i]))
    assert not CU.has_bit(c, rows)[i] and (c != m).sum() == 1
    z = np.zeros((3, 4), np.uint64)
    z[1, 2] = np.uint64(1) << np.uint64(1)    # row 129
    z[2, 3] = np.uint64(1) << np.uint64(63)   # row 255
    assert CU.bits_beyond(z, 129).tolist() == [1, 2] and CU.bits_beyond(z, 130).tolist() == [2] and CU.bits_beyond(z, 256).size == 0
    q = dict(apex=np.array([3]), row=np.array([9]), cell=np.array([[4, 2]]), tag=np.array(["centre"]))
    text = CU.describe(1, q, 0, np.arange(10)[::-1], np.array([2], np.uint32))
    assert "mode 1 apex 3 row 9 cell (iu, iv) (4, 2)" in text and "missing row 7 (flat index 2)" in text


def test_entries_refuse_bad_arguments_before_the_device(product_lib):
    """(no problem can be made without a GPU: what is left is the argument check in front of everything)"""
    import ctypes as C
    q, out = np.zeros((1, 8), np.float32), np.zeros((1, 10), np.uint32)
    f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    assert product_lib.hrt_debug_candidates(None, 0, 1, q.ctypes.data_as(f32p), out.ctypes.data_as(u32p)) == -1
    assert b"hrt_debug_candidates" in product_lib.hrt_last_error()
    npatch, kinds = C.c_uint64(), C.c_uint32()
    assert product_lib.hrt_debug_table_info(None, out.ctypes.data_as(u32p), q.ctypes.data_as(f32p), C.byref(npatch),
                                            C.byref(kinds)) == -1
