"""The GPU step of tests/test_gpu_candidates.py, a process of its own: python -m tests.candidates_child CASE.json OUT.npz

Builds the problem of one case (scene, endpoints; the environment carries HRT_TUNE / HRT_PATCH_MAX_BYTES), reads what
the tables were built with (hrt_debug_table_info), plants the queries of every mode the case asks for
(tests/candidates_util.py; the oracle's own sequences for the shadow and mirrored directions) and asks
hrt_debug_candidates for each lane's own lookup.  Everything -- queries, classes, returned words -- goes into OUT.npz;
the checks are the parent's.  A mode listed under "refused" must be refused by the entry (no table) without a launch."""
import ctypes as C
import json
import sys
import time

import numpy as np


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
    t0 = time.time()
    try:
        h = C.c_void_p()
        lib.check(L.hrt_problem_create(C.byref(scene), rx.ctypes.data_as(V3), tx.ctypes.data_as(V3), zr.ctypes.data_as(V3),
                                       zt.ctypes.data_as(V3), C.c_float(case["f_ghz"]), nrx, ntx, 0, C.byref(h)),
                  "hrt_problem_create")
    finally:
        abi.free_scene(scene)
    t_create = time.time() - t0
    T = int(L.hrt_problem_num_triangles(h))
    order = np.zeros(T, np.uint32)
    lib.check(L.hrt_problem_tri_order(h, order.ctypes.data_as(C.POINTER(C.c_uint32))), "hrt_problem_tri_order")
    info = abi.debug_table_info(L, h)
    flat = oracle.flatten(oracle.read_hrt(case["scene_path"]))
    rows_vtx = flat["tri_vtx"][order]
    out = dict(tri_order=order, nuv=info["nuv"], hmax=info["hmax"], ro_rx=info["ro_rx"], ro_img=info["ro_img"],
               num_patch=np.uint64(info["num_patch"]), kinds=np.uint32(info["kinds"]), t_create=t_create,
               num_rx=nrx, num_tx=ntx)
    u32 = lambda a: np.ascontiguousarray(a, np.uint32).view(np.float32)   # noqa: E731

    def run(mode, o, d, row, apex):
        q = np.concatenate([np.asarray(o, np.float32), np.asarray(d, np.float32), u32(row)[:, None], u32(apex)[:, None]], axis=1)
        t1 = time.time()
        got = abi.debug_candidates(L, h, mode, q)
        out["m%d_seconds" % mode] = time.time() - t1
        return got

    refused = []
    for mode in case.get("refused", []):
        try:
            abi.debug_candidates(L, h, mode, np.zeros((1, 8), np.float32))
        except RuntimeError as e:
            refused.append(mode)
            assert "no table" in str(e), e
    out["refused"] = np.asarray(refused, np.int64)

    modes = case["modes"]
    seed, spread = int(case.get("seed", 1)), int(case.get("spread", 2))
    if 0 in modes or 1 in modes:
        base = CU.patch_queries(rows_vtx, info["nuv"], info["hmax"], seed=seed, spread=spread)
        n = base["row"].size
        in_tab = base["row"] < T
        row_c = np.where(in_tab, base["row"], 0)
    if 0 in modes:
        apex = (np.arange(n) % nrx).astype(np.uint32)
        d = oracle.shadow_dirs(base["o"], rx[apex])
        got = run(0, base["o"], d, base["row"], apex)
        for k in ("row", "o", "cell", "centre", "cls", "tag"):
            out["m0_" + k] = base[k]
        out.update(m0_d=d, m0_apex=apex, m0_out=got)
    if 1 in modes:
        apex = (np.arange(n) % ntx).astype(np.uint32)
        d0, o_adv = oracle.mirror(flat, order[row_c], tx[apex], base["foot"], base["o"])
        var = CU.image_variants(CU.geometry(rows_vtx), row_c, o_adv, d0, tx[apex], info["ro_img"], seed=seed)
        s = var["src"]
        got = run(1, o_adv[s], var["d"], base["row"][s], apex[s])
        out.update(m1_row=base["row"][s], m1_o=o_adv[s], m1_d=var["d"], m1_apex=apex[s], m1_cell=base["cell"][s],
                   m1_centre=base["centre"][s], m1_tag=base["tag"][s], m1_kind=var["kind"], m1_factor=var["factor"],
                   m1_cls=CU.classes(CU.geometry(rows_vtx), info["nuv"], info["hmax"], base["row"][s], o_adv[s], T),
                   m1_out=got)
    if 2 in modes or 3 in modes:
        dirs, dtag = CU.direction_set(int(case.get("n_fib", 4096)))
    if 2 in modes:
        # the direction set from every TX, and every triangle's centroid aimed at (so that every row is some query's winner
        # unless it is hidden)
        cen = rows_vtx.reshape(-1, 3, 3).astype(np.float64).mean(axis=1).astype(np.float32)
        cen = cen[np.isfinite(cen).all(axis=1)]
        D, A, TG = [], [], []
        for t in range(ntx):
            aimed = oracle.shadow_dirs(np.tile(tx[t], (cen.shape[0], 1)), cen)
            D += [dirs, aimed]; A.append(np.full(dirs.shape[0] + aimed.shape[0], t)); TG += [dtag, np.full(aimed.shape[0], "aimed")]
        d, apex = np.concatenate(D), np.concatenate(A).astype(np.uint32)
        got = run(2, tx[apex], d, np.zeros(apex.size, np.uint32), apex)
        out.update(m2_o=tx[apex], m2_d=d, m2_apex=apex, m2_tag=np.concatenate(TG), m2_out=got)
    if 3 in modes:
        c, R = CU.region_ball(rows_vtx, tx)
        O, D, A, TG = [], [], [], []
        for t in range(ntx):   # launch rays: the origin IS the TX
            O.append(np.tile(tx[t], (dirs.shape[0], 1))); D.append(dirs); A.append(np.full(dirs.shape[0], nrx + t)); TG.append(dtag)
        _, pts = CU.points_on_triangles(rows_vtx, int(case.get("per_tri", 64)), seed=seed)
        for k in range(nrx):
            # shadow rays from points on the triangles, from the TXs, and along every direction of the set from a point
            # inside the region ball (the midpoint of the chord the line through the RX cuts out of 0.9 R)
            r = rx[k].astype(np.float64)
            dd = dirs.astype(np.float64)
            b = ((r - c) * dd).sum(axis=1)
            disc = b * b - (((r - c) ** 2).sum() - (0.9 * R) ** 2)
            ok = disc > 0
            s0, s1 = b - np.sqrt(np.where(ok, disc, 0.0)), b + np.sqrt(np.where(ok, disc, 0.0))   # o = r - s d inside for s in (s0, s1)
            ok &= s1 > 1e-2
            s = 0.5 * (np.maximum(s0, 1e-2) + s1)
            o_line = (r[None, :] - s[:, None] * dd)[ok].astype(np.float32)
            far = (c + np.array([3.0 * R, 0.0, 0.0])).astype(np.float32)[None, :]
            for name, o in (("on_tri", pts), ("at_tx", tx), ("line", o_line), ("outside_ball", far)):
                O.append(o); D.append(oracle.shadow_dirs(o, np.tile(rx[k], (o.shape[0], 1))))
                A.append(np.full(o.shape[0], k)); TG.append(dtag[ok] if name == "line" else np.full(o.shape[0], name))
        o, d, apex = np.concatenate(O), np.concatenate(D), np.concatenate(A).astype(np.uint32)
        got = run(3, o, d, np.zeros(apex.size, np.uint32), apex)
        dist = np.sqrt(((o.astype(np.float64) - c) ** 2).sum(axis=1))
        out.update(m3_o=o, m3_d=d, m3_apex=apex, m3_tag=np.concatenate(TG), m3_out=got,
                   m3_inside=dist <= 0.95 * R, m3_outside=dist >= 1.5 * R)
    L.hrt_problem_destroy(h)
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
