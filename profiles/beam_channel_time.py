"""What a beamformed channel costs on the device: Tracer.beam_channel next to the route without it, Tracer.array_channel
on every element pair followed by the contraction with the weights (torch, on the device).  C3 with a 4-element RX ULA
x 8 x 8 TX UPA at half a wavelength (256 element pairs), DFT codebooks of 4 x 16 beams (64 beam pairs), K = 1 024
subcarriers (30 kHz around the carrier), T in {1, 14}; then 16 x 16 by 16 x 16 elements with 8 x 8 beams, which the
array route refuses (2^26 element-domain points).

    python profiles/beam_channel_time.py [--config c3] [--k 1024] [--times 1,14] [--reps 3] [--no-large]
                                         [--out profiles/beam_channel/beam_channel_time_c3.json]

In ONE process: a Tracer traces the whole launch set once; per T, after a warm-up call of each route, (a) beam_channel
and (b) array_channel + einsum are timed with HIP events (`reps` calls each, median), and the two results are compared
within the tolerance of the tests: |a - b| <= 2e-5 ||W_rx[a]||_1 ||W_tx[b]||_1 sum_p |a_p^pol| (1e-5 for either
route).  Achieved FLOP of (a): 16 * unblocked scatter records * Br * Bt * T * K over its time (the GEMM alone: the
gains' work is not counted).  Kernel times by rocprof: run this under
`rocprofv3 --kernel-trace --stats -d <dir> -- python ...`."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import hermespy_rt_amd  # noqa: E402,F401
import torch  # noqa: E402  (HIP runtime first, see hermespy_rt_amd.lib)

from hermespy_rt_amd import beams  # noqa: E402
from hermespy_rt_amd import workloads as W  # noqa: E402
from hermespy_rt_amd.device import Tracer  # noqa: E402

PEAK_FP32 = 157.3e12
DF = 30e3
C0 = 299792458.0


def ula(n, d, axis):
    e = np.zeros((n, 3), np.float32)
    e[:, axis] = np.arange(n) * d
    return e


def upa(n1, n2, d):
    """n1 x n2 elements in the x-z plane"""
    e = np.zeros((n1 * n2, 3), np.float32)
    e[:, 0] = np.repeat(np.arange(n1), n2) * d
    e[:, 2] = np.tile(np.arange(n2), n1) * d
    return e


def upa_codebook(n1, n2, b1, b2):
    """b1 * b2 beams of an n1 x n2 UPA: Kronecker products of the first b1 / b2 rows of the DFT codebooks"""
    return np.kron(beams.dft_codebook(n1)[:b1], beams.dft_codebook(n2)[:b2]).astype(np.complex64)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def unblocked_records(tr):
    counts = tr.counts()
    return sum(int(tr.records(b, int(counts[b + 1]))["unblocked"].sum().item())
               for b in range(tr.nb) if int(counts[b + 1]))


def amplitude_sums(tr):
    """S[rx, tx, pol] = sum_p |a_p^pol| over the LoS entry and the unblocked records"""
    P = tr.paths()
    S = np.zeros((tr.nrx, tr.ntx, 2))
    link = (P["rx"] * tr.ntx + P["tx"]).cpu().numpy()
    for pol, k in enumerate(("a_te", "a_tm")):
        S[:, :, pol] = np.bincount(link, weights=P[k].abs().double().cpu().numpy(),
                                   minlength=tr.nrx * tr.ntx).reshape(tr.nrx, tr.ntx)
    L = tr.los()
    for rx in range(tr.nrx):
        for tx in range(tr.ntx):
            status = int(L[rx, tx][0:1].view(np.uint32)[0])
            S[rx, tx] += 1.0 if status == 0 else float(L[rx, tx][1]) if status == 2 else 0.0
    return S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--times", default="1,14")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-large", action="store_true", help="skip the 16 x 16 by 16 x 16 row")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    c = W.WORKLOADS[a.config]
    d = C0 / (c["f_ghz"] * 1e9) / 2
    K = a.k
    f0 = c["f_ghz"] * 1e9 - (K // 2) * DF
    tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"], c["num_paths"],
                c["num_bounces"])
    tr.trace()
    unblocked = unblocked_records(tr)
    S = amplitude_sums(tr)
    rows = []

    rxe, txe = ula(4, d, 1), upa(8, 8, d)
    wr, wt = beams.dft_codebook(4).astype(np.complex64), upa_codebook(8, 8, 4, 4)
    d_wr, d_wt = torch.from_numpy(wr).to(tr.device), torch.from_numpy(wt).to(tr.device)
    n1 = np.abs(wr).sum(axis=1)[:, None] * np.abs(wt).sum(axis=1)[None, :]
    for T in [int(x) for x in a.times.split(",")]:
        dt = 1e-3 if T > 1 else 0.0
        out_a = tr.beam_channel(rxe, txe, wr, wt, f0, DF, K, dt=dt, num_times=T)
        out_h = tr.array_channel(rxe, txe, f0, DF, K, dt=dt, num_times=T)

        def route_a():
            return tr.beam_channel(rxe, txe, wr, wt, f0, DF, K, dt=dt, num_times=T, out=out_a)

        def route_b():
            tr.array_channel(rxe, txe, f0, DF, K, dt=dt, num_times=T, out=out_h)
            return torch.einsum("ai,rtijpmk,bj->rtabpmk", d_wr.conj(), out_h, d_wt)

        ms_a, ms_b = timed(route_a, a.reps), timed(route_b, a.reps)
        err = (route_a() - route_b()).abs().amax(dim=(-2, -1)).double().cpu().numpy()   # (rx, tx, a, b, pol)
        lim = 2e-5 * n1[None, None, :, :, None] * S[:, :, None, None, :]
        flop = 16.0 * unblocked * wr.shape[0] * wt.shape[0] * K * T
        t = statistics.median(ms_a) * 1e-3
        row = dict(config=a.config, Nr=len(rxe), Nt=len(txe), Br=wr.shape[0], Bt=wt.shape[0], K=K, T=T,
                   unblocked_records=unblocked, beam_channel_ms=statistics.median(ms_a), beam_channel_ms_all=ms_a,
                   array_then_contract_ms=statistics.median(ms_b), array_then_contract_ms_all=ms_b,
                   speedup=statistics.median(ms_b) / statistics.median(ms_a),
                   max_err_over_bound=float((err / lim).max()), agree=bool((err <= lim).all()),
                   flop=flop, tflops=flop / t / 1e12, peak_share=flop / t / PEAK_FP32)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del out_a, out_h
        torch.cuda.empty_cache()

    if not a.no_large:
        rxe = txe = upa(16, 16, d)
        wr = wt = upa_codebook(16, 16, 2, 4)
        refused = None
        try:
            tr.array_channel(rxe, txe, f0, DF, K)
        except ValueError as e:
            refused = str(e)
        out_a = tr.beam_channel(rxe, txe, wr, wt, f0, DF, K)
        ms_a = timed(lambda: tr.beam_channel(rxe, txe, wr, wt, f0, DF, K, out=out_a), a.reps)
        flop = 16.0 * unblocked * wr.shape[0] * wt.shape[0] * K
        t = statistics.median(ms_a) * 1e-3
        row = dict(config=a.config, Nr=len(rxe), Nt=len(txe), Br=wr.shape[0], Bt=wt.shape[0], K=K, T=1,
                   unblocked_records=unblocked, beam_channel_ms=statistics.median(ms_a), beam_channel_ms_all=ms_a,
                   array_channel_refused=refused, finite=bool(torch.isfinite(torch.view_as_real(out_a)).all()),
                   flop=flop, tflops=flop / t / 1e12, peak_share=flop / t / PEAK_FP32)
        rows.append(row)
        print(json.dumps(row), flush=True)
    tr.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    if not all(r.get("agree", True) for r in rows):
        sys.exit("the two routes disagree beyond the tolerance")


if __name__ == "__main__":
    main()
