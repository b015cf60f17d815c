"""What the per-point equalizers cost: hrt_channel_equalizer on the array channel of C3 (4 links, 1 time sample, 1 024
subcarriers: 8 192 points) at 8 x 8 and at 64 x 16 elements, both kinds, with and without W, next to
torch.linalg.solve on H^H H + lambda I and torch.linalg.pinv on the same device tensor (gathered to [points, Nr, Nt]
outside the timed region) and next to the array_channel call that produced H; then the same sizes on standard-normal
matrices (full rank: a traced channel close to rank one is singular for zero-forcing, and says so in `status`).

    python profiles/channel_equalizer_time.py [--shapes 8x8,64x16] [--reps 3]
                                              [--out profiles/equalizer/channel_equalizer_time.json]

Every shape runs in a child process of its own under a time limit (a child that hangs or faults ends the run: nothing
more is started).  Per shape: the launch set is traced once; one warm-up call, then HIP events around each of `reps`
calls, the median reported.  The SINR of the two is compared where torch gives one (largest |difference| / (1 + sinr)
over the regular points).  Where this build of torch has no batched routine on the device, or refuses a singular
matrix, the row says so instead of a time.  None of the comparisons is a pass condition."""
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


def one_tensor(torch, tr, H, n0, reps, res, tag):
    """the device calls and torch's on one tensor -> res[tag + ...]"""
    nrx, ntx, nr, nt = (int(v) for v in H.shape[:4])
    out = {(k, w): tr.equalizer(H, n0, k, w)["buffer"] for k in ("lmmse", "zf") for w in (True, False)}
    for k in ("lmmse", "zf"):
        res[tag + k + "_ms"], res[tag + k + "_all_ms"] = timed(
            torch, lambda: tr.equalizer(H, n0, k, True, out=out[k, True]), reps)
        res[tag + k + "_sinr_only_ms"], _ = timed(torch, lambda: tr.equalizer(H, n0, k, False, out=out[k, False]), reps)
        st = tr.equalizer(H, n0, k, False)["status"]
        res[tag + k + "_singular"], res[tag + k + "_nonfinite"] = int((st == 1).sum()), int((st == 2).sum())
    A = H.permute(0, 1, 4, 5, 6, 2, 3).reshape(-1, nr, nt).contiguous()
    AH = A.mH.contiguous()
    eye = torch.eye(nt, dtype=A.dtype, device=A.device)
    for k, lam in (("lmmse", n0), ("zf", 0.0)):
        try:
            res[tag + "torch_solve_" + k + "_ms"], _ = timed(torch, lambda: torch.linalg.solve(AH @ A + lam * eye, AH), reps)
        except Exception as e:   # no batched solve on the device in this build of torch, or a singular matrix
            res[tag + "torch_solve_" + k] = "unavailable: %s" % (str(e).splitlines()[0][:200],)
    try:
        res[tag + "torch_pinv_ms"], _ = timed(torch, lambda: torch.linalg.pinv(A), reps)
    except Exception as e:
        res[tag + "torch_pinv"] = "unavailable: %s" % (str(e).splitlines()[0][:200],)
    try:
        G = torch.linalg.inv((AH @ A + n0 * eye).to(torch.complex128))
        rho = 1.0 / (n0 * torch.diagonal(G, dim1=1, dim2=2).real) - 1.0
        got = tr.equalizer(H, n0, "lmmse", False)["sinr"].permute(0, 1, 3, 4, 5, 2).reshape(-1, nt).double()
        res[tag + "lmmse_sinr_difference"] = float(((got - rho).abs() / (1 + rho)).max())
    except Exception as e:
        res[tag + "lmmse_sinr_difference"] = "unavailable: %s" % (str(e).splitlines()[0][:200],)


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
    # the noise: a quarter of the largest |H|_F^2 of a point (the strongest link at about 6 dB per stream)
    n0 = float((H.abs() ** 2).sum((2, 3)).max()) / 4
    res["noise"] = n0
    one_tensor(torch, tr, H, n0, reps, res, "")
    # the same sizes on standard-normal matrices: full rank, so zero-forcing is regular
    g = torch.Generator(device=H.device).manual_seed(7)
    Hn = torch.randn(H.shape, dtype=torch.complex64, device=H.device, generator=g)
    one_tensor(torch, tr, Hn, 1.0, reps, res, "normal_")
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
