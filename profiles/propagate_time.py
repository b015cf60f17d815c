"""What applying taps to waveforms costs: hrt_propagate on planted tensors against the same contraction written in
torch on the same device (per block, torch.nn.functional.conv1d on the real and imaginary planes).

    python profiles/propagate_time.py [--shapes mfma_8x8,mfma_1x1,general] [--reps 3] [--out FILE.json]

Shapes (standard-normal taps and samples, l_min = 0, N = N_out - L + 1):
    mfma_8x8   nrx = 4, ntx = 1, Nr = Nt = 8, L = 256, S = 1024, N_out = 65 536 (M = 64)      MFMA form
    mfma_1x1   the same with Nr = Nt = 1                                                       MFMA form
    general    nrx = 4, ntx = 1, Nr = Nt = 8, L = 64, S = 1, N_out = 4 096 (M = 4 096)         general form
Every shape runs in a child process of its own under a time limit (a child that hangs or faults ends the run: nothing
more is started).  Per shape: one warm-up call, then HIP events around each of `reps` calls, the median reported; the
torch form is timed the same way, its weights (flipped taps in the 2 x 2 real embedding) prepared outside the timed
region.  FLOP = 8 R K N_out with R = nrx Nr 2 complex rows and K = ntx Nt L complex reductions; the share is of the
157.3 TF/s f32-matrix peak.  The two results are compared (largest difference over the largest value)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PEAK_FP32 = 157.3e12
SHAPES = {
    "mfma_8x8": dict(nrx=4, ntx=1, nr=8, nt=8, L=256, S=1024, n_out=65536),
    "mfma_1x1": dict(nrx=4, ntx=1, nr=1, nt=1, L=256, S=1024, n_out=65536),
    "general": dict(nrx=4, ntx=1, nr=8, nt=8, L=64, S=1, n_out=4096),
}
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


def run_shape(name, reps):
    import hermespy_rt_amd  # noqa: F401
    import torch  # (HIP runtime first, see hermespy_rt_amd.lib)
    from hermespy_rt_amd import abi, lib

    s = SHAPES[name]
    nrx, ntx, nr, nt, L, S, n_out = (s[k] for k in ("nrx", "ntx", "nr", "nt", "L", "S", "n_out"))
    M, N = -(-n_out // S), n_out - L + 1
    R, P = nrx * nr * 2, ntx * nt
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    h = torch.randn((nrx, ntx, nr, nt, 2, M, L), dtype=torch.complex64, device=dev, generator=g)
    x = torch.randn((ntx, nt, N), dtype=torch.complex64, device=dev, generator=g)
    y = torch.empty((nrx, nr, 2, n_out), dtype=torch.complex64, device=dev)
    Lb = lib.load()
    spec = abi.propagate_spec(nrx, ntx, nr, nt, M, L, 0, S, N, n_out)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def ours():
        abi.run_propagate(Lb, 0, spec, h.data_ptr(), x.data_ptr(), y.data_ptr(), 0, stream)

    ms, all_ms = timed(torch, ours, reps)
    flop = 8.0 * R * (P * L) * n_out
    res = dict(shape=s, M=M, N=N, R=R, K=P * L, form="general" if (M > 1 and S % 16) else "mfma", ms=ms, all_ms=all_ms,
               tflops=flop / (ms * 1e-3) / 1e12, peak_share=flop / (ms * 1e-3) / PEAK_FP32)

    # the torch form: rows (rx, i, pol) x (re, im), channels (tx, j) x (re, im), per block a conv1d over the window
    hr = h.permute(0, 2, 4, 1, 3, 5, 6).reshape(R, P, M, L).flip(-1)           # [R, P, M, L], taps reversed
    w = torch.cat([torch.cat([hr.real, -hr.imag], 1), torch.cat([hr.imag, hr.real], 1)], 0)   # [2R, 2P, M, L]
    w = w.permute(2, 0, 1, 3).contiguous()                                    # [M, 2R, 2P, L]
    xr = torch.cat([x.reshape(P, N).real, x.reshape(P, N).imag], 0)           # [2P, N]
    xp = torch.nn.functional.pad(xr, (L - 1, n_out + S)).unsqueeze(0)         # sample k of x at column k + L - 1
    yt = torch.empty((2 * R, n_out), dtype=torch.float32, device=dev)

    def theirs():
        for m in range(M):
            lo, hi = m * S, min((m + 1) * S, n_out)
            yt[:, lo:hi] = torch.nn.functional.conv1d(xp[:, :, lo:hi + L - 1], w[m])[0]

    tms, tall = timed(torch, theirs, reps)
    res.update(torch_ms=tms, torch_all_ms=tall, torch_tflops=flop / (tms * 1e-3) / 1e12)
    yr = torch.complex(yt[:R], yt[R:]).reshape(nrx, nr, 2, n_out)
    res["difference"] = float((y - yr).abs().max() / yr.abs().max())
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
        print("%-9s %-7s %9.3f ms  %6.2f TF/s  %5.1f %% of peak   torch %9.3f ms  %6.2f TF/s   difference %.2e"
              % (name, r["form"], r["ms"], r["tflops"], 100 * r["peak_share"], r["torch_ms"], r["torch_tflops"],
                 r["difference"]), flush=True)
    try:
        commit = subprocess.check_output(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], text=True,
                                         stderr=subprocess.DEVNULL).strip()
    except Exception:
        commit = None
    doc = dict(device="MI355X", peak_fp32_matrix=PEAK_FP32, commit=commit, reps=a.reps, results=results)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
