"""What the array taps of a dominant-path list cost: on C3 (4 links, 1 time sample, 256 taps: 2 048 points) at 8 x 8 and
at 64 x 16 elements, for K = 64 and K = 1 024, the time of dominant_paths(K) and of sparse_array_taps on its result,
next to array_taps on the same trace (the sum over all records), next to the same contraction from the list in torch
(phases in float64, sinc in float64, einsum in complex64), and how far the list's taps are from the whole ones:
|h - h_sparse|_F / |h|_F with dominant.captured_fraction.

    python profiles/sparse_taps_time.py [--shapes 8x8,64x16] [--reps 3] [--out profiles/sparse/sparse_taps_time.json]

Every shape runs in a child process of its own under a time limit (a child that hangs or faults ends the run: nothing
more is started).  Per shape: the launch set is traced once; one warm-up call, then HIP events around each of `reps`
calls, the median reported.  None of the comparisons is a pass condition."""
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
KS = (64, 1024)
L, L_MIN, T, FS = 256, 0, 1, 122.88e6
C0 = 299792458.0
STEP_LIMIT_S = 400


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


def torch_composition(torch, dp, rxe, txe, fa, fc, l, t):
    """the definition from the list's device views: phases and sinc arguments in float64, the phases reduced to a
    revolution, exp, sinc weights and einsum in float32 / complex64 -> [nrx, ntx, Nr, Nt, 2, T, L]"""
    kept = dp["kept"]
    nrx, ntx, P = dp["tau"].shape
    live = (torch.arange(P, device=kept.device) < kept[..., None]).to(torch.complex64)
    amp = torch.stack([dp["a_te"], dp["a_tm"]], -1) * live[..., None]                          # [r, t, p, 2]
    tau, nu = dp["tau"].double(), dp["freq_shift"].double()
    ph = nu[..., None] * t - fc * tau[..., None]                                                # [r, t, p, T]
    W = torch.polar(torch.ones_like(ph, dtype=torch.float32), (2 * np.pi * (ph - ph.round())).float())
    V = torch.sinc(l - FS * tau[..., None]).float().to(torch.complex64)                         # [r, t, p, L]
    d = (dp["u_rx"].double() @ rxe.T)[..., :, None] + (dp["u_tx"].double() @ txe.T)[..., None, :]   # [r, t, p, Nr, Nt]
    sp = fa / C0 * d
    S = torch.polar(torch.ones_like(sp, dtype=torch.float32), (2 * np.pi * (sp - sp.round())).float())
    return torch.einsum("rtpij,rtpq,rtpm,rtpl->rtijqml", S, amp, W, V)


def run_shape(name, reps):
    import hermespy_rt_amd  # noqa: F401
    import torch  # (HIP runtime first, see hermespy_rt_amd.lib)
    from hermespy_rt_amd import dominant
    from hermespy_rt_amd import workloads as W
    from hermespy_rt_amd.device import Tracer

    nr, nt = SHAPES[name]
    c = W.WORKLOADS["c3"]
    fa = c["f_ghz"] * 1e9
    d = C0 / fa / 2
    rxe, txe = upa(nr, d), upa(nt, d)
    tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"], c["num_paths"],
                c["num_bounces"])
    tr.trace()
    H = tr.array_taps(rxe, txe, FS, L, L_MIN, num_times=T)
    res = dict(Nr=nr, Nt=nt, links=tr.nrx * tr.ntx, L=L, l_min=L_MIN, T=T, fs_hz=FS, points=tr.nrx * tr.ntx * 2 * T * L)
    res["array_taps_ms"], res["array_taps_all_ms"] = timed(
        torch, lambda: tr.array_taps(rxe, txe, FS, L, L_MIN, num_times=T, out=H), reps)
    hn = float(torch.linalg.vector_norm(H))
    moments = tr.power_profiles(0.0, 1e-9, 1)["moments"]
    l = torch.as_tensor(L_MIN + np.arange(L), device=tr.device).double()
    t = torch.zeros(T, dtype=torch.float64, device=tr.device)
    rt, tt = torch.as_tensor(rxe, device=tr.device).double(), torch.as_tensor(txe, device=tr.device).double()
    for k in KS:
        r = {}
        dp = tr.dominant_paths(k)
        r["dominant_paths_ms"], _ = timed(torch, lambda: tr.dominant_paths(k, out=dp["buffer"]), reps)
        Hs = tr.sparse_array_taps(dp, rxe, txe, FS, L, L_MIN, fa, num_times=T)
        r["sparse_array_taps_ms"], r["sparse_array_taps_all_ms"] = timed(
            torch, lambda: tr.sparse_array_taps(dp, rxe, txe, FS, L, L_MIN, fa, num_times=T, out=Hs), reps)
        r["kept"] = dp["kept"].cpu().numpy().astype(np.int64).ravel().tolist()
        r["eligible"] = dp["eligible"].cpu().numpy().astype(np.int64).ravel().tolist()
        r["relative_error_to_array_taps"] = float(torch.linalg.vector_norm(H - Hs)) / hn
        r["captured_fraction"] = dominant.captured_fraction(dp, moments).ravel().tolist()
        try:
            Ht = torch_composition(torch, dp, rt, tt, fa, fa, l, t)
            r["torch_composition_ms"], _ = timed(torch, lambda: torch_composition(torch, dp, rt, tt, fa, fa, l, t), reps)
            r["relative_difference_to_torch"] = float(torch.linalg.vector_norm(Ht - Hs) / torch.linalg.vector_norm(Hs))
            del Ht
        except Exception as e:   # (out of memory at the largest shape, or an operator this build lacks)
            r["torch_composition"] = "unavailable: %s" % (str(e).splitlines()[0][:200],)
        res["K%d" % k] = r
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
