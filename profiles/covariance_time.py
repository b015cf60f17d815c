"""What the spatial covariance matrices cost: hermespy_rt.compute_array_covariance against hermespy_rt.compute_paths,
the covariance kernels' device time and their error at full size, on C3 (or any workload) with Nr = Nt = 64 (8 x 8 UPAs
at half a wavelength), both sides, LoS and scatter.

    python profiles/covariance_time.py [--configs c3] [--reps 5] [--out profiles/covariance/covariance_time_c3.json]

In ONE process, per config: after a warm-up call of each, the two drop-in calls alternate (`reps` times each) and the
median wall times are reported (--no-drop-in skips them); then a Tracer traces the whole launch set once and a whole
hrt_array_covariance call is timed with HIP events around each of `reps` calls.  FLOP: every unblocked record issues,
per side, 16 MFMAs (4 x 2 tiles of 16 x 32, two polarisations) of 2 * 32 * 32 * 2 FLOP per 64 x 64 block of the upper
triangle; the share of the f32-MFMA peak (64 FLOP / clk / SIMD) is that over the call's time.  Error (--no-error skips
it): the largest |R - R64| / trace(R64) * N per side against a float64 sum of the same records formed with torch on
the device (the steering in float64 from the float directions and offsets).
Kernel times by rocprof: run this under `rocprofv3 --kernel-trace --stats -d <dir> -- python ...`."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import hermespy_rt_amd  # noqa: E402
import torch  # noqa: E402,F401  (HIP runtime first, see hermespy_rt_amd.lib)

sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
import hermespy_rt  # noqa: E402

from hermespy_rt_amd import lib as _lib  # noqa: E402
from hermespy_rt_amd import workloads as W  # noqa: E402
from hermespy_rt_amd.device import Tracer  # noqa: E402

PEAK_FP32 = 157.3e12
C0 = 299792458.0
FLOP_PER_BLOCK = 16 * 2 * 32 * 32 * 2


def upa(n1, n2, d):
    """n1 x n2 elements in the x-z plane"""
    e = np.zeros((n1 * n2, 3), np.float32)
    e[:, 0] = np.repeat(np.arange(n1), n2) * d
    e[:, 2] = np.tile(np.arange(n2), n1) * d
    return e


def drop_in_args(c):
    return (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], len(c["rx_pos"]),
            len(c["tx_pos"]), c["num_paths"], c["num_bounces"])


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def blocks(n):
    nb = (n + 63) // 64
    return nb * (nb + 1) // 2


def launch_dirs(tr):
    """departure direction of every global path (hrt_launch_dirs_host of the whole launch set)"""
    s = _lib.Shard(tr.num_paths, 0, 1, 0, tr.nb)
    d = np.empty((tr.num_paths, 3), np.float32)
    _lib.check(tr.L.hrt_launch_dirs_host(C.byref(s), d.ctypes.data_as(C.POINTER(C.c_float)), 0))
    return torch.from_numpy(d).to(tr.device)


def reference(tr, rxe, txe, fa, chunk=1 << 18):
    """R_rx, R_tx [nrx, ntx, 2, N, N] complex128 on the device: float64 sums over tr.paths() and the LoS entries"""
    P = tr.paths()
    dirs = launch_dirs(tr)
    el = [torch.from_numpy(e.astype(np.float64)).to(tr.device) for e in (rxe, txe)]
    R = [torch.zeros((tr.nrx * tr.ntx, 2, e.shape[0], e.shape[0]), dtype=torch.complex128, device=tr.device)
         for e in el]
    link = P["rx"] * tr.ntx + P["tx"]

    def add(side, lk, p, u):
        ph = (fa / C0) * (u.double() @ el[side].T)
        s = torch.exp(2j * np.pi * (ph - torch.round(ph)))
        for pol in range(2):
            R[side][lk, pol] += (p[pol][:, None] * s).T @ s.conj()

    for lk in range(tr.nrx * tr.ntx):
        idx = torch.nonzero(link == lk)[:, 0]
        for i in range(0, idx.numel(), chunk):
            s = idx[i:i + chunk]
            p = [P[k][s].real.double() ** 2 + P[k][s].imag.double() ** 2 for k in ("a_te", "a_tm")]
            add(0, lk, p, P["direction_rx"][s])
            add(1, lk, p, dirs[P["path"][s]])
    L = tr.los()
    for rx in range(tr.nrx):
        for tx in range(tr.ntx):
            e = L[rx, tx]
            status = int(e[0:1].view(np.uint32)[0])
            if status == 1:
                continue
            a = 1.0 if status == 0 else float(e[1])
            u = np.array([-1.0, 0.0, 0.0]) if status == 0 else np.asarray(e[3:6], np.float64)
            u = torch.from_numpy(u[None, :]).to(tr.device)
            p = [torch.full((1,), a * a, dtype=torch.float64, device=tr.device)] * 2
            add(0, rx * tr.ntx + tx, p, -u)
            add(1, rx * tr.ntx + tx, p, u)
    return [r.reshape(tr.nrx, tr.ntx, 2, r.shape[-1], r.shape[-1]) for r in R]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3")
    ap.add_argument("--n1", type=int, default=8, help="the arrays are n1 x n2 UPAs")
    ap.add_argument("--n2", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-drop-in", action="store_true", help="device times only")
    ap.add_argument("--no-error", action="store_true", help="no float64 reference")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.configs.split(","):
        c = W.WORKLOADS[name]
        args = drop_in_args(c)
        fa = c["f_ghz"] * 1e9
        rxe = txe = upa(a.n1, a.n2, C0 / fa / 2)
        n = rxe.shape[0]
        row = dict(config=name, Nr=n, Nt=n)
        if not a.no_drop_in:
            cv = lambda: hermespy_rt.compute_array_covariance(*args, rx_elements=rxe, tx_elements=txe)  # noqa: E731
            dp = lambda: hermespy_rt.compute_paths(*args)  # noqa: E731
            cv()
            dp()
            tc, td = [], []
            for _ in range(a.reps):
                tc.append(wall(cv)[0])
                td.append(wall(dp)[0])
            row.update(compute_array_covariance_s=statistics.median(tc), compute_array_covariance_all_s=tc,
                       compute_paths_s=statistics.median(td), compute_paths_all_s=td)
            row["ratio"] = row["compute_array_covariance_s"] / row["compute_paths_s"]
            hermespy_rt.cache_clear()
        tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"],
                    c["num_paths"], c["num_bounces"])
        tr.trace()
        records = int(tr.work()["records"])
        unblocked = int(tr.paths(nonzero_only=False)["unblocked"].sum().item())
        out = tr.array_covariance(rxe, txe)["buffer"]
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.array_covariance(rxe, txe, out=out)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        flop = float(FLOP_PER_BLOCK) * unblocked * 2 * blocks(n)
        t = statistics.median(ms) * 1e-3
        row.update(links=tr.nrx * tr.ntx, records=records, unblocked=unblocked, call_ms=statistics.median(ms),
                   call_ms_all=ms, flop=flop, tflops=flop / t / 1e12, peak_share=flop / t / PEAK_FP32)
        if not a.no_error:
            got = tr.array_covariance(rxe, txe)
            for side, ref in zip(("rx", "tx"), reference(tr, rxe, txe, fa)):
                scale = torch.diagonal(ref, dim1=-2, dim2=-1).real.mean(dim=-1)[..., None, None]   # sum_p p
                err = (got[side].to(torch.complex128) - ref).abs() / scale.clamp_min(1e-300)
                row["max_rel_err_" + side] = float(err.max().item())
        tr.close()
        del tr, out
        torch.cuda.empty_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
