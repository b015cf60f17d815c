"""What the codebook selection costs: hrt_codebook_select on standard-normal tensors of array_channel's layout with
8 192 points (4 links, 1 time sample, 1 024 subcarriers), subbands of 12, next to the same search in torch on the same
device tensors: einsum to [points, C, Nr, L], the Gram matrices, torch.linalg.det (or the squared norm under "power"),
the mean over the subband, argmax.

    shape       H         codebook
    4x32-dp2    4 x 32    codebook.dual_polarised(16, 4, layers=2)   128 entries of rank 2
    2x8-dp1     2 x 8     codebook.dual_polarised(4, 4, layers=1)    64 entries of rank 1
    16x64-r4    16 x 64   1 024 random entries of rank 4 and unit norm

    python profiles/codebook_select_time.py [--shapes 4x32-dp2,2x8-dp1,16x64-r4] [--reps 3]
                                            [--out profiles/codebook/codebook_select_time.json]

Every shape runs in a child process of its own under a time limit (a child that hangs or faults ends the run: nothing
more is started).  Per row: one warm-up call, then HIP events around each of `reps` calls, the median reported, both
metrics, bare and with table and effective.  torch's chain is cut into blocks of subbands where its intermediate
would not fit (the blocks are part of its time).  The indices of the two are compared (the share of subbands that
agree; the two co-phases of a rank-2 dual-polarised entry tie mathematically, so that row agrees up to the co-phase).
Where this build of torch has no batched determinant on the device the row says so instead of a time.  None of the
comparisons is a pass condition."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {"4x32-dp2": (4, 32, ("dual", 16, 4, 2)), "2x8-dp1": (2, 8, ("dual", 4, 4, 1)),
          "16x64-r4": (16, 64, ("random", 1024, 4))}
LINKS, T, K, S = 4, 1, 1024, 12
NOISE = 0.25
BLOCK_BYTES = 1 << 30           # torch's [points, C, Nr, L] intermediate per block
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


def torch_select(torch, A, W, metric, eye, bands, block):
    """the same search in torch: A [subbands-major points, Nr, Nt] grouped as [B, n, Nr, Nt] per band list entry"""
    best = []
    for X in bands:                                   # X [b, n, Nr, Nt]: subbands of equal length
        for i in range(0, X.shape[0], block):
            E = torch.einsum("bnit,ctl->bncil", X[i:i + block], W)
            if metric == "power":
                f = (E.abs() ** 2).sum((-2, -1))
            else:
                G = E.mH @ E / NOISE + eye
                f = torch.log2(torch.linalg.det(G).real)
            best.append(f.mean(1).argmax(1))
    return torch.cat(best)


def run_shape(name, reps):
    import hermespy_rt_amd  # noqa: F401
    import torch  # (HIP runtime first, see hermespy_rt_amd.lib)
    from hermespy_rt_amd import codebook as CB
    from hermespy_rt_amd import workloads as WL
    from hermespy_rt_amd.device import Tracer

    nr, nt, cb = SHAPES[name]
    c = dict(WL.WORKLOADS["c1"], num_paths=64)          # the selection reads only its tensors: nothing is traced
    tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"], c["num_paths"],
                c["num_bounces"])
    dev = tr.device
    g = torch.Generator(device=dev).manual_seed(7)
    H = torch.randn((LINKS, 1, nr, nt, 2, T, K), dtype=torch.complex64, device=dev, generator=g)
    if cb[0] == "dual":
        Wn = CB.dual_polarised(cb[1], cb[2], cb[3]).astype(np.complex64)
    else:
        rng = np.random.default_rng(3)
        Wn = rng.standard_normal((cb[1], nt, cb[2])) + 1j * rng.standard_normal((cb[1], nt, cb[2]))
        Wn = (Wn / np.sqrt((np.abs(Wn) ** 2).sum((1, 2), keepdims=True))).astype(np.complex64)
    W = torch.from_numpy(Wn).to(dev)
    Cn, L = int(W.shape[0]), int(W.shape[2])
    Kk = int(H.shape[6])
    res = dict(Nr=nr, Nt=nt, L=L, C=Cn, points=LINKS * 2 * T * Kk, K=Kk, S=S, subbands=LINKS * 2 * T * ((Kk + S - 1) // S),
               noise=NOISE, intermediate_bytes=LINKS * 2 * T * Kk * Cn * nr * L * 8)
    # torch's operands, gathered outside the timed region: [groups, K, Nr, Nt] -> full subbands and the short last one
    A = H.permute(0, 1, 4, 5, 6, 2, 3).reshape(-1, Kk, nr, nt)
    full = (Kk // S) * S
    bands = [A[:, :full].reshape(-1, S, nr, nt).contiguous()]
    if full < Kk:
        bands.append(A[:, full:].contiguous())
    eye = torch.eye(L, dtype=W.dtype, device=dev)
    block = max(1, BLOCK_BYTES // (S * Cn * nr * L * 8))
    for metric in ("power", "capacity"):
        for tag, table, eff in (("", False, False), ("_table_effective", True, True)):
            out = tr.codebook_select(H, W, metric, NOISE, S, table, eff)["buffer"]
            res[metric + tag + "_ms"], res[metric + tag + "_all_ms"] = timed(
                torch, lambda: tr.codebook_select(H, W, metric, NOISE, S, table, eff, out=out), reps)
        r = tr.codebook_select(H, W, metric, NOISE, S)
        res[metric + "_flagged"] = int((r["status"] != 0).sum())
        try:
            res["torch_" + metric + "_ms"], _ = timed(torch, lambda: torch_select(torch, A, W, metric, eye, bands, block),
                                                      reps)
            want = torch_select(torch, A, W, metric, eye, bands, block)
            nb = (Kk + S - 1) // S
            idx = r["index"].reshape(-1, nb).to(torch.int64)
            got = torch.cat([idx[:, :full // S].reshape(-1)] + ([idx[:, -1]] if full < Kk else []))
            res[metric + "_index_agreement"] = float((got == want).double().mean())
            if cb[0] == "dual" and cb[3] == 2:
                res[metric + "_beam_agreement"] = float((got // 2 == want // 2).double().mean())
        except Exception as e:   # no batched determinant on the device in this build of torch
            res["torch_" + metric] = "unavailable: %s" % (str(e).splitlines()[0][:200],)
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
