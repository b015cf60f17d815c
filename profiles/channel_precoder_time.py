"""What the per-point precoders cost: hrt_channel_precoder on the array channel of C3 (4 links, 1 time sample, 1 024
subcarriers: 8 192 points) at 8 x 8 and at 16 x 64 elements (streams x transmit elements), all three kinds, with and
without P, next to the same computation in torch on the same device tensor (gathered to [points, Nr, Nt] outside the
timed region): torch.linalg.solve on H H^H + alpha I, the products, the normalisation and the SINR; and next to the
array_channel call that produced H.  Then the same sizes on standard-normal matrices (full rank: a traced channel close
to rank one is singular for zero-forcing, and says so in `status`).

    python profiles/channel_precoder_time.py [--shapes 8x8,16x64] [--reps 3]
                                             [--out profiles/precoder/channel_precoder_time.json]

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

SHAPES = {"8x8": (8, 8), "16x64": (16, 64)}
KINDS = ("mrt", "zf", "rzf")
K, T, DF = 1024, 1, 30e3
C0 = 299792458.0
POWER = 1.0
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


def torch_precoder(torch, A, AH, eye, kind, alpha, n0):
    """the same computation in torch on [points, Nr, Nt]: P (TOTAL normalisation) and the SINR"""
    if kind == "mrt":
        P0 = AH
    else:
        P0 = torch.linalg.solve(A @ AH + alpha * eye, A).mH       # (H H^H + alpha I)^-1 H, transposed: Hermitian Gram
    P = P0 * torch.sqrt(POWER / (P0.abs() ** 2).sum((1, 2)))[:, None, None]
    p = (A @ P).abs() ** 2
    sig = torch.diagonal(p, dim1=1, dim2=2)
    return P, sig / (p.sum(2) - sig + n0)


def one_tensor(torch, tr, H, n0, reps, res, tag):
    """the device calls and torch's on one tensor -> res[tag + ...]"""
    nrx, ntx, nr, nt = (int(v) for v in H.shape[:4])
    alpha = nr * n0 / POWER
    out = {(k, w): tr.precoder(H, n0, k, POWER, weights=w)["buffer"] for k in KINDS for w in (True, False)}
    for k in KINDS:
        res[tag + k + "_ms"], res[tag + k + "_all_ms"] = timed(
            torch, lambda: tr.precoder(H, n0, k, POWER, weights=True, out=out[k, True]), reps)
        res[tag + k + "_sinr_only_ms"], _ = timed(
            torch, lambda: tr.precoder(H, n0, k, POWER, weights=False, out=out[k, False]), reps)
        st = tr.precoder(H, n0, k, POWER, weights=False)["status"]
        res[tag + k + "_singular"], res[tag + k + "_nonfinite"] = int((st == 1).sum()), int((st == 2).sum())
    res[tag + "stream_rzf_ms"], _ = timed(torch, lambda: tr.precoder(H, n0, "rzf", POWER, normalize="stream"), reps)
    A = H.permute(0, 1, 4, 5, 6, 2, 3).reshape(-1, nr, nt).contiguous()
    AH = A.mH.contiguous()
    eye = torch.eye(nr, dtype=A.dtype, device=A.device)
    for k in KINDS:
        a = alpha if k == "rzf" else 0.0
        try:
            res[tag + "torch_" + k + "_ms"], _ = timed(torch, lambda: torch_precoder(torch, A, AH, eye, k, a, n0), reps)
            rho = torch_precoder(torch, A.to(torch.complex128), AH.to(torch.complex128), eye.to(torch.complex128), k, a,
                                 n0)[1]
            r = tr.precoder(H, n0, k, POWER, weights=False)
            got = r["sinr"].permute(0, 1, 3, 4, 5, 2).reshape(-1, nr).double()
            ok = (r["status"].reshape(-1) == 0) & torch.isfinite(rho).all(1)
            res[tag + k + "_sinr_difference"] = float(((got - rho).abs() / (1 + rho))[ok].max()) if bool(ok.any()) \
                else "no regular point"
        except Exception as e:   # no batched solve on the device in this build of torch, or a singular matrix
            res[tag + "torch_" + k] = "unavailable: %s" % (str(e).splitlines()[0][:200],)


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
    res = dict(Nr=nr, Nt=nt, links=tr.nrx * tr.ntx, K=K, T=T, points=tr.nrx * tr.ntx * 2 * T * K, power=POWER)
    res["array_channel_ms"], _ = timed(torch, lambda: tr.array_channel(rxe, txe, f0, DF, K, num_times=T, out=H), reps)
    # the noise: a quarter of the largest |H|_F^2 of a point
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
