"""What the maximum-likelihood detection costs: hrt_channel_detect on standard-normal tensors of array_channel's layout
with 8 192 points (4 links, 1 time sample, 1 024 subcarriers), next to the same search in torch on the same device
tensors: the hypotheses' symbol vectors [Q, Nt] once, then per block of points the broadcast to [points, Q, Nr], the
squared distances, argmin, and with LLRs the two masked minima per bit.

    shape      Nr  Nt  B   Q
    2x2-b2      2   2  2     16
    4x4-b2      4   4  2    256
    4x2-b6      4   2  6  4 096
    4x3-b4      4   3  4  4 096
    16x6-b2    16   6  2  4 096

    python profiles/detect_time.py [--shapes 2x2-b2,4x4-b2,4x2-b6,4x3-b4,16x6-b2] [--reps 3]
                                   [--out profiles/detect/detect_time.json]

Every shape runs in a child process of its own under a time limit (a child that hangs or faults ends the run: nothing
more is started).  Per row: one warm-up call, then HIP events around each of `reps` calls, the median reported, with
and without LLRs.  torch's chain is cut into blocks of points whose [points, Q, Nr] intermediate stays within 1 GB
(the blocks are part of its time).  The indices of the two are compared (the share of points that agree).  None of
the comparisons is a pass condition."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {"2x2-b2": (2, 2, 2), "4x4-b2": (4, 4, 2), "4x2-b6": (4, 2, 6), "4x3-b4": (4, 3, 4), "16x6-b2": (16, 6, 2)}
LINKS, T, K = 4, 1, 1024
NOISE = 0.25
BLOCK_BYTES = 1 << 30           # torch's [points, Q, Nr] intermediate per block
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


def torch_detect(torch, A, y, X, masks, block, llr):
    """the same search in torch: A [points, Nr, Nt], y [points, Nr], X [Q, Nt], masks [Nt B, Q] (bit is 1)"""
    best, llrs = [], []
    inf = torch.tensor(float("inf"), device=A.device)
    for i in range(0, A.shape[0], block):
        E = torch.einsum("pit,qt->pqi", A[i:i + block], X)
        d = ((y[i:i + block, None, :] - E).abs() ** 2).sum(-1)              # [p, Q]
        best.append(d.argmin(1))
        if llr:
            m1 = torch.where(masks[None], d[:, None, :], inf).amin(-1)
            m0 = torch.where(masks[None], inf, d[:, None, :]).amin(-1)
            llrs.append((m0 - m1) / NOISE)
    return torch.cat(best), (torch.cat(llrs) if llr else None)


def run_shape(name, reps):
    import hermespy_rt_amd  # noqa: F401
    import torch  # (HIP runtime first, see hermespy_rt_amd.lib)
    from hermespy_rt_amd import detect as DT
    from hermespy_rt_amd import workloads as WL
    from hermespy_rt_amd.device import Tracer

    nr, nt, B = SHAPES[name]
    c = dict(WL.WORKLOADS["c1"], num_paths=64)          # the detection reads only its tensors: nothing is traced
    tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"], c["num_paths"],
                c["num_bounces"])
    dev = tr.device
    g = torch.Generator(device=dev).manual_seed(7)
    Q = 1 << (nt * B)
    Sn = DT.qam(B).astype(np.complex64)
    S = torch.from_numpy(Sn).to(dev)
    H = torch.randn((LINKS, 1, nr, nt, 2, T, K), dtype=torch.complex64, device=dev, generator=g)
    sent = torch.randint(0, Q, (LINKS, 1, 2, T, K), device=dev, generator=g)
    digits = (sent[..., None] >> (torch.arange(nt, device=dev) * B)) & ((1 << B) - 1)
    Y = torch.einsum("abitpmk,abpmkt->abipmk", H, S[digits])
    Y = (Y + (NOISE ** 0.5) * torch.randn(Y.shape, dtype=torch.complex64, device=dev, generator=g)).contiguous()
    points = LINKS * 2 * T * K
    res = dict(Nr=nr, Nt=nt, B=B, Q=Q, points=points, noise=NOISE, intermediate_bytes=points * Q * nr * 8)
    # torch's operands, gathered outside the timed region
    A = H.permute(0, 1, 4, 5, 6, 2, 3).reshape(-1, nr, nt).contiguous()
    y = Y.permute(0, 1, 3, 4, 5, 2).reshape(-1, nr).contiguous()
    q = torch.arange(Q, device=dev)
    X = S[(q[:, None] >> (torch.arange(nt, device=dev) * B)) & ((1 << B) - 1)]
    pos = torch.tensor([j * B + (B - 1 - b) for j in range(nt) for b in range(B)], device=dev)
    masks = ((q[None, :] >> pos[:, None]) & 1).bool()
    block = max(1, BLOCK_BYTES // (Q * nr * 8))
    for tag, llr in (("", False), ("_llr", True)):
        out = tr.detect(H, Y, S, NOISE, llr)["buffer"]
        res["detect" + tag + "_ms"], res["detect" + tag + "_all_ms"] = timed(
            torch, lambda: tr.detect(H, Y, S, NOISE, llr, out=out), reps)
        res["torch" + tag + "_ms"], _ = timed(torch, lambda: torch_detect(torch, A, y, X, masks, block, llr), reps)
    r = tr.detect(H, Y, S, NOISE, True)
    res["flagged"] = int((r["status"] != 0).sum())
    want, wl = torch_detect(torch, A, y, X, masks, block, True)
    res["index_agreement"] = float((r["index"].reshape(-1).to(torch.int64) == want).double().mean())
    res["sent_decided"] = float((r["index"].to(torch.int64) == sent).double().mean())
    got = r["llr"].permute(0, 1, 4, 5, 6, 2, 3).reshape(points, nt * B)
    res["llr_max_abs_difference"] = float((got - wl).abs().max())
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
