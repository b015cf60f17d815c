"""The GPU step of tests/test_gpu_candidates_pencil.py, a process of its own:
    python -m tests.candidates_pencil_child CASE.json OUT.npz

Builds the problem of one case (the environment carries HRT_TUNE), plants rays where the pencil bounds of the patch
masks (csrc/hrt_kernels.hip pencil_culls, DESIGN_ACCEL.md A.5 items 4-6) are tightest and asks hrt_debug_candidates
for each lane's own lookup.  Queries and returned words go into OUT.npz; the checks are the parent's.

  corner   the 8 corners and 12 edge midpoints of a cell's prism at the served limits: cell coordinates on the cell's
           borders, 1 / 64 cell outside the grid where the cell lies on its rim, |h| = hmax - 1e-5;
  graze    cells whose centre sees the RX at under 2 degrees above their plane: the centre and the four cell corners;
  edge     origins on whatever surface the line from an RX through a point 1 mm either side of a small triangle's edge
           midpoints and vertices meets: behind that point (the small triangle lies between origin and RX) and on the
           other side of the RX (it lies beyond the RX);
  image    (mode 1) the corner and graze origins as mirrored rays of every TX, the unperturbed line and lines that pass
           the image at 0.5 / 0.9 / 1.1 / 2 x ro_img (tests/candidates_util.py image_variants)."""
import ctypes as C
import json
import sys

import numpy as np

LIMIT_OUT = 1.0 / 64
N_CORNER, N_GRAZE, N_SMALL, N_IMAGE = 3000, 150, 25, 1000


def prism_points(lo_u, hi_u, lo_v, hi_v, hlim):
    """the 8 corners and 12 edge midpoints of [lo_u, hi_u] x [lo_v, hi_v] x [-hlim, hlim]"""
    us, vs, hs = (lo_u, 0.5 * (lo_u + hi_u), hi_u), (lo_v, 0.5 * (lo_v + hi_v), hi_v), (-hlim, 0.0, hlim)
    out = []
    for a in range(3):
        for b in range(3):
            for c in range(3):
                if (a == 1) + (b == 1) + (c == 1) <= 1:
                    out.append((us[a], vs[b], hs[c]))
    return out


def plant(CU, oracle, flat, order, rows_vtx, nuv, hmax, rx, seed):
    rng = np.random.default_rng(seed)
    g = CU.geometry(rows_vtx)
    T = g["v1"].shape[0]
    nrx = rx.shape[0]
    hlim = float(hmax) - 1e-5
    served = np.flatnonzero(nuv[:, 0] > 0)
    row, FU, FV, H, apex, tag = [], [], [], [], [], []
    # ---- corner ----
    per_tri = max(1, N_CORNER // (20 * max(served.size, 1)))
    for j in served:
        nu, nv = int(nuv[j, 0]), int(nuv[j, 1])
        cells = CU.pick_cells(nu, nv, rng, spread=1)
        for (iu, iv) in [cells[k] for k in rng.permutation(len(cells))[:per_tri]]:
            lo_u, hi_u = (iu - LIMIT_OUT if iu == 0 else iu), (iu + 1 + LIMIT_OUT if iu == nu - 1 else iu + 1)
            lo_v, hi_v = (iv - LIMIT_OUT if iv == 0 else iv), (iv + 1 + LIMIT_OUT if iv == nv - 1 else iv + 1)
            for (fu, fv, h) in prism_points(lo_u, hi_u, lo_v, hi_v, hlim):
                row.append(j); FU.append(fu); FV.append(fv); H.append(h); apex.append(len(row) % nrx); tag.append("corner")
    # ---- graze ----
    J, IU, IV = [], [], []
    for j in served:
        nu, nv = int(nuv[j, 0]), int(nuv[j, 1])
        iu, iv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
        J.append(np.full(iu.size, j)); IU.append(iu.reshape(-1)); IV.append(iv.reshape(-1))
    J, IU, IV = np.concatenate(J), np.concatenate(IU), np.concatenate(IV)
    cen = g["v1"][J] + ((IU + 0.5) / nuv[J, 0])[:, None] * g["e1"][J] + ((IV + 0.5) / nuv[J, 1])[:, None] * g["e2"][J]
    n_graze = 0
    for k in range(nrx):
        w = rx[k].astype(np.float64)[None, :] - cen
        dist = np.sqrt((w * w).sum(axis=1))
        with np.errstate(invalid="ignore", divide="ignore"):
            sin_el = np.abs((w * g["n"][J]).sum(axis=1)) / dist
        ok = np.flatnonzero((sin_el < np.sin(np.radians(2.0))) & (dist > 1.0))
        for i in rng.permutation(ok)[:N_GRAZE]:
            for (du, dv) in ((0.5, 0.5), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)):
                row.append(J[i]); FU.append(IU[i] + du); FV.append(IV[i] + dv); H.append(1e-4); apex.append(k); tag.append("graze")
                n_graze += 1
    row = np.asarray(row, np.int64)
    nuf = nuv[row].astype(np.float64)
    foot = g["v1"][row] + (np.asarray(FU) / nuf[:, 0])[:, None] * g["e1"][row] + (np.asarray(FV) / nuf[:, 1])[:, None] * g["e2"][row]
    o = (foot + np.asarray(H)[:, None] * g["n"][row]).astype(np.float32)
    foot = foot.astype(np.float32)
    # ---- edge ----
    longest = np.sqrt(np.maximum.reduce([(g["e1"] ** 2).sum(axis=1), (g["e2"] ** 2).sum(axis=1), ((g["e2"] - g["e1"]) ** 2).sum(axis=1)]))
    small = np.flatnonzero(np.isfinite(g["n"]).all(axis=1) & (longest < 3.0))
    small = small[rng.permutation(small.size)[:N_SMALL]]
    targets = []
    for j in small:
        v = [g["v1"][j], g["v1"][j] + g["e1"][j], g["v1"][j] + g["e2"][j]]
        c = (v[0] + v[1] + v[2]) / 3.0
        for a in range(3):
            mid = 0.5 * (v[a] + v[(a + 1) % 3])
            e = v[(a + 1) % 3] - v[a]
            p = np.cross(g["n"][j], e)
            p /= np.sqrt((p * p).sum())
            out = v[a] - c
            out /= np.sqrt((out * out).sum())
            targets += [mid + 1e-3 * p, mid - 1e-3 * p, v[a] + 1e-3 * out, v[a] - 1e-3 * out]
    e_row, e_o, e_apex, e_tag = [], [], [], []
    if targets:
        tg = np.asarray(targets)
        inv = np.zeros(T, np.int64)
        inv[order] = np.arange(T)
        for k in range(nrx):
            r = rx[k].astype(np.float64)
            d = tg - r[None, :]
            L = np.sqrt((d * d).sum(axis=1))
            d = d / L[:, None]
            for sgn, start, name in ((1.0, tg + 2e-3 * d, "edge_before"), (-1.0, np.tile(r, (tg.shape[0], 1)) - 2e-3 * d, "edge_beyond")):
                s32, d32 = start.astype(np.float32), (sgn * d).astype(np.float32)
                tri, dist = oracle.closest_hits(flat, s32, d32)
                hit = tri != 0xFFFFFFFF
                t = dist.view(np.float32).astype(np.float64)
                oo = s32.astype(np.float64) + t[:, None] * d32.astype(np.float64)
                e_row.append(inv[np.where(hit, tri, 0)][hit]); e_o.append(oo[hit].astype(np.float32))
                e_apex.append(np.full(int(hit.sum()), k)); e_tag += [name] * int(hit.sum())
    if e_row:
        er = np.concatenate(e_row)
        row, o, foot = np.concatenate([row, er]), np.concatenate([o, np.concatenate(e_o)]), np.concatenate([foot, np.concatenate(e_o)])
        apex = np.concatenate([np.asarray(apex, np.int64), np.concatenate(e_apex)])
        tag = tag + e_tag
    q = dict(row=row.astype(np.uint32), o=o, foot=foot, apex=np.asarray(apex, np.uint32), tag=np.asarray(tag))
    q["cls"] = CU.classes(g, nuv, hmax, row, o, T)
    return q


def main(case_path, out_path):
    case = json.load(open(case_path))
    from hermespy_rt_amd import abi, lib
    from oracle import oracle

    from . import candidates_util as CU
    L = lib.load()
    rx = np.ascontiguousarray(np.asarray(case["rx_pos"], np.float32).reshape(-1, 3))
    tx = np.ascontiguousarray(np.asarray(case["tx_pos"], np.float32).reshape(-1, 3))
    nrx, ntx = rx.shape[0], tx.shape[0]
    zr, zt = np.zeros_like(rx), np.zeros_like(tx)
    V3 = C.POINTER(abi.Vec3)
    scene = L.scene_load(str(case["scene_path"]).encode())
    try:
        h = C.c_void_p()
        lib.check(L.hrt_problem_create(C.byref(scene), rx.ctypes.data_as(V3), tx.ctypes.data_as(V3), zr.ctypes.data_as(V3),
                                       zt.ctypes.data_as(V3), C.c_float(case["f_ghz"]), nrx, ntx, 0, C.byref(h)),
                  "hrt_problem_create")
    finally:
        abi.free_scene(scene)
    T = int(L.hrt_problem_num_triangles(h))
    order = np.zeros(T, np.uint32)
    lib.check(L.hrt_problem_tri_order(h, order.ctypes.data_as(C.POINTER(C.c_uint32))), "hrt_problem_tri_order")
    info = abi.debug_table_info(L, h)
    flat = oracle.flatten(oracle.read_hrt(case["scene_path"]))
    rows_vtx = flat["tri_vtx"][order]
    out = dict(tri_order=order, nuv=info["nuv"], hmax=info["hmax"], ro_img=info["ro_img"], num_patch=np.uint64(info["num_patch"]))
    u32 = lambda a: np.ascontiguousarray(a, np.uint32).view(np.float32)   # noqa: E731

    def run(mode, o, d, row, apex):
        q = np.concatenate([np.asarray(o, np.float32), np.asarray(d, np.float32), u32(row)[:, None], u32(apex)[:, None]], axis=1)
        return abi.debug_candidates(L, h, mode, q)

    base = plant(CU, oracle, flat, order, rows_vtx, info["nuv"], info["hmax"], rx, int(case.get("seed", 3)))
    d = oracle.shadow_dirs(base["o"], rx[base["apex"]])
    out.update(m0_row=base["row"], m0_o=base["o"], m0_d=d, m0_apex=base["apex"], m0_tag=base["tag"], m0_cls=base["cls"],
               m0_out=run(0, base["o"], d, base["row"], base["apex"]))
    # mode 1: the corner and graze origins as rays that left a TX and were mirrored on their triangle
    pick = np.flatnonzero(np.isin(base["tag"], ("corner", "graze")))
    pick = pick[np.random.default_rng(5).permutation(pick.size)[:N_IMAGE]]
    apex = (np.arange(pick.size) % ntx).astype(np.uint32)
    rows1 = base["row"][pick]
    d0, o_adv = oracle.mirror(flat, order[rows1], tx[apex], base["foot"][pick], base["o"][pick])
    g = CU.geometry(rows_vtx)
    var = CU.image_variants(g, rows1.astype(np.int64), o_adv, d0, tx[apex], info["ro_img"], seed=7)
    s = var["src"]
    out.update(m1_row=rows1[s], m1_o=o_adv[s], m1_d=var["d"], m1_apex=apex[s], m1_tag=base["tag"][pick][s], m1_kind=var["kind"],
               m1_factor=var["factor"], m1_cls=CU.classes(g, info["nuv"], info["hmax"], rows1[s], o_adv[s], T),
               m1_out=run(1, o_adv[s], var["d"], rows1[s], apex[s]))
    L.hrt_problem_destroy(h)
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
