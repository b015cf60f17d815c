"""What the per-point SVD costs: hrt_channel_svd on the array channel of C3 (4 links, 1 time sample, 1 024
subcarriers: 8 192 points) at 8 x 8 and at 64 x 16 elements, with and without vectors, next to torch.linalg.svd /
torch.linalg.svdvals on the same device tensor (gathered to [points, Nr, Nt] outside the timed region) and next to
the array_channel call that produced H; then the same sizes on standard-normal matrices (full rank: a traced channel
close to rank one is finished after one sweep, these need several).

    python profiles/channel_svd_time.py [--shapes 8x8,64x16] [--reps 3] [--out profiles/svd/channel_svd_time.json]

Every shape runs in a child process of its own under a time limit (a child that hangs or faults ends the run: nothing
more is started).  Per shape: the launch set is traced once; one warm-up call, then HIP events around each of `reps`
calls, the median reported.  The singular values of the two are compared (largest difference over sigma_0).  Where
this build of torch has no batched SVD on the device, the row says so instead of a time."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {"8x8": (8, 8), "64x16": (64, 16)}
K, T, DF = 1024, 1, 30e3
C0 = 299792458.0
STEP_LIMIT_S = 240


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def upa(n, d):
    """n elements at spacing d: a ULA along y up to 8, else an (n / 8) x 8 UPA in the y-z plane"""
    e = np.zeros((n, 3), np.float32)
    e[:, 1] = (np.arange(n) % 8) * d
    e[:, 2] = (np.arange(n) // 8) * d
    return e


def run_shape(name, reps):
    import hermespy_rt_amd  # noqa: F401
    import torch  # (HIP runtime first, see hermespy_rt_amd.lib)
    from hermespy_rt_amd import workloads as W
    from hermespy_rt_amd.device import Tracer

    nr, nt = SHAPES[name]
    c = W.WORKLOADS["c3"]
    d = C0 / (c["f_ghz"] * 1e9) / 2
    rxe, txe = upa(nr, d), upa(nt, d)
    f0 = c["f_ghz"] * 1e9 - (K // 2) * DF
    tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"], c["num_paths"],
                c["num_bounces"])
    tr.trace()
    H = tr.array_channel(rxe, txe, f0, DF, K, num_times=T)
    res = dict(Nr=nr, Nt=nt, links=tr.nrx * tr.ntx, K=K, T=T, points=tr.nrx * tr.ntx * 2 * T * K)
    res["array_channel_ms"], _ = timed(torch, lambda: tr.array_channel(rxe, txe, f0, DF, K, num_times=T, out=H), reps)
    out = {v: tr.svd(H, v)["buffer"] for v in (True, False)}
    res["svd_ms"], res["svd_all_ms"] = timed(torch, lambda: tr.svd(H, True, out=out[True]), reps)
    res["svdvals_ms"], res["svdvals_all_ms"] = timed(torch, lambda: tr.svd(H, False, out=out[False]), reps)
    r = tr.svd(H, False)
    sweeps = r["sweeps"]
    res["sweeps_max"] = int(sweeps.max())
    res["not_converged"] = int((sweeps < 0).sum())
    A = H.permute(0, 1, 4, 5, 6, 2, 3).reshape(-1, nr, nt).contiguous()
    try:
        res["torch_svd_ms"], _ = timed(torch, lambda: torch.linalg.svd(A, full_matrices=False), reps)
        res["torch_svdvals_ms"], _ = timed(torch, lambda: torch.linalg.svdvals(A), reps)
        s = torch.linalg.svdvals(A).reshape(tr.nrx, tr.ntx, 2, T, K, min(nr, nt)).permute(0, 1, 5, 2, 3, 4)
        res["difference"] = float(((r["sigma"] - s).abs().amax(2) / s[:, :, 0].clamp_min(1e-30)).max())
    except Exception as e:   # no batched SVD on the device in this build of torch
        res["torch"] = "unavailable: %s" % (str(e).splitlines()[0][:200],)
    # the same sizes on standard-normal matrices: full rank, so the sweeps a traced channel does not need are made
    g = torch.Generator(device=H.device).manual_seed(7)
    Hn = torch.randn(H.shape, dtype=torch.complex64, device=H.device, generator=g)
    res["normal_svd_ms"], _ = timed(torch, lambda: tr.svd(Hn, True, out=out[True]), reps)
    res["normal_svdvals_ms"], _ = timed(torch, lambda: tr.svd(Hn, False, out=out[False]), reps)
    rn = tr.svd(Hn, False)
    res["normal_sweeps_max"] = int(rn["sweeps"].max())
    res["normal_not_converged"] = int((rn["sweeps"] < 0).sum())
    An = Hn.permute(0, 1, 4, 5, 6, 2, 3).reshape(-1, nr, nt).contiguous()
    try:
        res["normal_torch_svd_ms"], _ = timed(torch, lambda: torch.linalg.svd(An, full_matrices=False), reps)
        res["normal_torch_svdvals_ms"], _ = timed(torch, lambda: torch.linalg.svdvals(An), reps)
        s = torch.linalg.svdvals(An).reshape(tr.nrx, tr.ntx, 2, T, K, min(nr, nt)).permute(0, 1, 5, 2, 3, 4)
        res["normal_difference"] = float(((rn["sigma"] - s).abs().amax(2) / s[:, :, 0]).max())
    except Exception as e:
        res["normal_torch"] = "unavailable: %s" % (str(e).splitlines()[0][:200],)
    tr.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(run_shape(a.child, a.reps)))
        return 0
    results = {}
    for name in a.shapes.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps)],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print("%s: no result within %d s; stopping" % (name, STEP_LIMIT_S))
            return 1
        if p.returncode != 0:
            print("%s failed (%d); stopping\n%s" % (name, p.returncode, p.stderr[-2000:]))
            return 1
        r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        results[name] = r
        print(name, json.dumps(r), flush=True)
    try:
        commit = subprocess.check_output(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], text=True,
                                         stderr=subprocess.DEVNULL).strip()
    except Exception:
        commit = None
    doc = dict(device="MI355X", commit=commit, reps=a.reps, results=results)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
