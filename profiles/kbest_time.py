"""What the K-best tree-search detection costs: hrt_channel_kbest on standard-normal tensors of array_channel's layout
with 8 192 points (4 links, 1 time sample, 1 024 subcarriers), sorted QR, with LLRs, next to the same per-level chain
in torch on the same device tensors: a batched QR of the column-sorted H, then per level the children's partial
distances as a [points, K M] tensor and `topk` over it, and the list LLRs from the final list.

    shape        Nr  Nt  B   K
    4x4-b4-k16    4   4  4  16
    4x4-b6-k64    4   4  6  64
    8x8-b2-k32    8   8  2  32
    4x2-b6-k64    4   2  6  64     (the one shape Tracer.detect accepts as well: its time is reported next to it)

    python profiles/kbest_time.py [--shapes 4x4-b4-k16,...] [--reps 3] [--out profiles/kbest/kbest_time.json]

Every shape runs in a child process of its own under a time limit (a child that hangs or faults ends the run: nothing
more is started).  Per row: one warm-up call, then HIP events around each of `reps` calls, the median reported.  The
kernel is timed twice, as built and with HRT_KBEST_NO_SKIP=1 (every batch sorted and merged; a child process of its
own, the variable is read at every call), and the two outputs are compared byte for byte.  torch's chain orders the
columns by their norms once (not per step) and breaks ties as topk does, so its indices are compared as the share of
points that agree.  None of the comparisons is a pass condition."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = {"4x4-b4-k16": (4, 4, 4, 16), "4x4-b6-k64": (4, 4, 6, 64), "8x8-b2-k32": (8, 8, 2, 32),
          "4x2-b6-k64": (4, 2, 6, 64)}
LINKS, T, K = 4, 1, 1024
NOISE, CLIP = 0.05, 50.0
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


def torch_kbest(torch, A, y, S, B, k):
    """the per-level topk chain in torch: A [points, Nr, Nt], y [points, Nr] -> index [points], llr [points, Nt B]"""
    P, nr, nt = A.shape
    M = S.shape[0]
    order = (A.abs() ** 2).sum(1).argsort(1)                                   # weakest column first
    Q, R = torch.linalg.qr(torch.gather(A, 2, order[:, None, :].expand(P, nr, nt)))
    z = torch.einsum("pij,pi->pj", Q.conj(), y)
    rho = ((y.abs() ** 2).sum(1) - (z.abs() ** 2).sum(1)).clamp_min(0)
    ped = rho[:, None]
    key = torch.zeros((P, 1), dtype=torch.int64, device=A.device)
    sym = torch.zeros((P, 1, nt), dtype=torch.int64, device=A.device)        # by position
    x = torch.arange(M, device=A.device)
    for i in range(nt - 1, -1, -1):
        b = z[:, i, None] - torch.einsum("pt,plt->pl", R[:, i, i + 1:], S[sym[:, :, i + 1:]])
        e = b[:, :, None] - R[:, i, i, None, None] * S[None, None, :]
        cp = (ped[:, :, None] + e.abs() ** 2).reshape(P, -1)
        keep = min(k, cp.shape[1])
        ped, at = torch.topk(cp, keep, dim=1, largest=False)
        parent, digit = at // M, at % M
        sym = torch.gather(sym, 1, parent[:, :, None].expand(P, keep, nt)).clone()
        sym[:, :, i] = digit
        key = torch.gather(key, 1, parent) | (digit << (order[:, i, None] * B))
    best = ped.argmin(1)
    index = torch.gather(key, 1, best[:, None])[:, 0]
    pos = torch.tensor([j * B + (B - 1 - b) for j in range(nt) for b in range(B)], device=A.device)
    one = ((key[:, None, :] >> pos[None, :, None]) & 1).bool()                # [P, Nt B, list]
    inf = torch.tensor(float("inf"), device=A.device)
    m1 = torch.where(one, ped[:, None, :], inf).amin(-1)
    m0 = torch.where(one, inf, ped[:, None, :]).amin(-1)
    llr = ((m0 - m1) / NOISE).nan_to_num(posinf=CLIP, neginf=-CLIP).clamp(-CLIP, CLIP)
    return index, llr


def run_shape(name, reps):
    import hermespy_rt_amd  # noqa: F401
    import torch  # (HIP runtime first, see hermespy_rt_amd.lib)
    from hermespy_rt_amd import detect as DT
    from hermespy_rt_amd import workloads as WL
    from hermespy_rt_amd.device import Tracer

    nr, nt, B, k = SHAPES[name]
    c = dict(WL.WORKLOADS["c1"], num_paths=64)          # the detection reads only its tensors: nothing is traced
    tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"], c["num_paths"],
                c["num_bounces"])
    dev = tr.device
    g = torch.Generator(device=dev).manual_seed(7)
    Sn = DT.qam(B).astype(np.complex64)
    S = torch.from_numpy(Sn).to(dev)
    H = torch.randn((LINKS, 1, nr, nt, 2, T, K), dtype=torch.complex64, device=dev, generator=g)
    hi = torch.randint(0, 1 << 30, (2, LINKS, 1, 2, T, K), device=dev, generator=g)
    sent = ((hi[0] << 30) | hi[1]) & ((1 << (nt * B)) - 1)
    digits = (sent[..., None] >> (torch.arange(nt, device=dev) * B)) & ((1 << B) - 1)
    Y = torch.einsum("abitpmk,abpmkt->abipmk", H, S[digits])
    Y = (Y + (NOISE ** 0.5) * torch.randn(Y.shape, dtype=torch.complex64, device=dev, generator=g)).contiguous()
    points = LINKS * 2 * T * K
    res = dict(Nr=nr, Nt=nt, B=B, K=k, points=points, noise=NOISE, clip=CLIP,
               skip=os.environ.get("HRT_KBEST_NO_SKIP") != "1")
    out = tr.kbest(H, Y, S, NOISE, k, CLIP)["buffer"]
    res["kbest_ms"], res["kbest_all_ms"] = timed(torch, lambda: tr.kbest(H, Y, S, NOISE, k, CLIP, out=out), reps)
    bare = tr.kbest(H, Y, S, NOISE, k, CLIP, llr=False)["buffer"]
    res["kbest_no_llr_ms"], _ = timed(torch, lambda: tr.kbest(H, Y, S, NOISE, k, CLIP, llr=False, out=bare), reps)
    r = tr.kbest(H, Y, S, NOISE, k, CLIP)
    torch.cuda.synchronize()
    import hashlib
    res["sha256"] = hashlib.sha256(r["buffer"].cpu().numpy().tobytes()).hexdigest()
    res["flagged"] = int((r["status"] == 1).sum())
    res["deficient"] = int((r["status"] == 2).sum())
    index = r["index"].to(torch.int64) & 0xFFFFFFFF
    res["sent_decided"] = float((index == sent).double().mean())
    if res["skip"]:
        A = H.permute(0, 1, 4, 5, 6, 2, 3).reshape(-1, nr, nt).contiguous()
        y = Y.permute(0, 1, 3, 4, 5, 2).reshape(-1, nr).contiguous()
        res["torch_ms"], _ = timed(torch, lambda: torch_kbest(torch, A, y, S, B, k), reps)
        want, wl = torch_kbest(torch, A, y, S, B, k)
        res["index_agreement"] = float((index.reshape(-1) == want).double().mean())
        got = r["llr"].permute(0, 1, 4, 5, 6, 2, 3).reshape(points, nt * B)
        res["llr_median_abs_difference"] = float((got - wl).abs().median())
        if nt * B <= 12:
            d = tr.detect(H, Y, S, NOISE, True)
            dout = d["buffer"]
            res["detect_ms"], _ = timed(torch, lambda: tr.detect(H, Y, S, NOISE, True, out=dout), reps)
            res["detect_index_agreement"] = float((d["index"] == r["index"]).double().mean())
    tr.close()
    return res


def child(name, reps, no_skip):
    env = dict(os.environ)
    env.pop("HRT_KBEST_NO_SKIP", None)
    if no_skip:
        env["HRT_KBEST_NO_SKIP"] = "1"
    return subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(reps)],
                          capture_output=True, text=True, timeout=STEP_LIMIT_S, env=env)


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
        for no_skip in (False, True):
            try:
                p = child(name, a.reps, no_skip)
            except subprocess.TimeoutExpired:
                print("%s: no result within %d s; stopping" % (name, STEP_LIMIT_S))
                return 1
            if p.returncode != 0:
                print("%s failed (%d); stopping\n%s" % (name, p.returncode, p.stderr[-2000:]))
                return 1
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            if no_skip:
                results[name]["kbest_no_skip_ms"] = r["kbest_ms"]
                results[name]["same_bytes_without_skip"] = r["sha256"] == results[name]["sha256"]
            else:
                results[name] = r
        print(name, json.dumps(results[name]), flush=True)
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
