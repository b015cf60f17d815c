"""What beamformed taps cost on the device: Tracer.beam_taps next to the route without it, Tracer.array_taps on every
element pair followed by the contraction with the weights (torch, on the device).  The setup of
profiles/beam_channel_time.py: C3 with a 4-element RX ULA x 8 x 8 TX UPA at half a wavelength (256 element pairs), DFT
codebooks of 4 x 16 beams (64 beam pairs), f_s = 122.88 MHz, f_c = f_a = the carrier; (T, L) in {(1, 256), (64, 64)};
then 16 x 16 by 16 x 16 elements with 8 x 8 beams at L = 512, which the array route refuses (2^25 element-domain
points).

    python profiles/beam_taps_time.py [--config c3] [--shapes 1x256,64x64] [--reps 3] [--no-large]
                                      [--out profiles/beam_taps/beam_taps_time_c3.json]

In ONE process: a Tracer traces the whole launch set once; per shape, after a warm-up call of each route, (a) beam_taps
and (b) array_taps + einsum are timed alternately with HIP events (`reps` calls each, median), and the two results are
compared within the tolerance of the tests: |a - b| <= 2e-5 ||W_rx[a]||_1 ||W_tx[b]||_1 sum_p |a_p^pol| (1e-5 for
either route).  Achieved FLOP of (a): 8 * unblocked scatter records * Br * Bt * T * L over its time (the GEMM alone:
the gains' work is not counted).  Kernel times by rocprof: run this under
`rocprofv3 --kernel-trace --stats -d <dir> -- python ...`.  Exit status 1 if the routes disagree or (a) is not faster
than (b)."""
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

from beam_channel_time import amplitude_sums, ula, unblocked_records, upa, upa_codebook  # noqa: E402

PEAK_FP32 = 157.3e12
FS = 122.88e6
C0 = 299792458.0


def timed_pair(fa, fb, reps):
    """the two routes warmed once each, then timed alternately: ([ms of a], [ms of b])"""
    out = ([], [])
    for fn in (fa, fb):
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for ms, fn in zip(out, (fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--shapes", default="1x256,64x64", help="T x L, comma separated")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-large", action="store_true", help="skip the 16 x 16 by 16 x 16 row")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    c = W.WORKLOADS[a.config]
    d = C0 / (c["f_ghz"] * 1e9) / 2
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
    for T, L in [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]:
        dt = 1e-4 if T > 1 else 0.0
        out_a = tr.beam_taps(rxe, txe, wr, wt, FS, L, dt=dt, num_times=T)
        out_h = tr.array_taps(rxe, txe, FS, L, dt=dt, num_times=T)

        def route_a():
            return tr.beam_taps(rxe, txe, wr, wt, FS, L, dt=dt, num_times=T, out=out_a)

        def route_b():
            tr.array_taps(rxe, txe, FS, L, dt=dt, num_times=T, out=out_h)
            return torch.einsum("ai,rtijpml,bj->rtabpml", d_wr.conj(), out_h, d_wt)

        ms_a, ms_b = timed_pair(route_a, route_b, a.reps)
        err = (route_a() - route_b()).abs().amax(dim=(-2, -1)).double().cpu().numpy()   # (rx, tx, a, b, pol)
        lim = 2e-5 * n1[None, None, :, :, None] * S[:, :, None, None, :]
        flop = 8.0 * unblocked * wr.shape[0] * wt.shape[0] * T * L
        t = statistics.median(ms_a) * 1e-3
        row = dict(config=a.config, Nr=len(rxe), Nt=len(txe), Br=wr.shape[0], Bt=wt.shape[0], T=T, L=L,
                   unblocked_records=unblocked, beam_taps_ms=statistics.median(ms_a), beam_taps_ms_all=ms_a,
                   array_then_contract_ms=statistics.median(ms_b), array_then_contract_ms_all=ms_b,
                   speedup=statistics.median(ms_b) / statistics.median(ms_a),
                   faster=bool(statistics.median(ms_a) < statistics.median(ms_b)),
                   max_err_over_bound=float((err / lim).max()), agree=bool((err <= lim).all()),
                   flop=flop, tflops=flop / t / 1e12, peak_share=flop / t / PEAK_FP32)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del out_a, out_h
        torch.cuda.empty_cache()

    if not a.no_large:
        rxe = txe = upa(16, 16, d)
        wr = wt = upa_codebook(16, 16, 2, 4)
        L = 512
        refused = None
        try:
            tr.array_taps(rxe, txe, FS, L)
        except ValueError as e:
            refused = str(e)
        out_a = tr.beam_taps(rxe, txe, wr, wt, FS, L)
        ms_a, _ = timed_pair(lambda: tr.beam_taps(rxe, txe, wr, wt, FS, L, out=out_a), lambda: None, a.reps)
        flop = 8.0 * unblocked * wr.shape[0] * wt.shape[0] * L
        t = statistics.median(ms_a) * 1e-3
        row = dict(config=a.config, Nr=len(rxe), Nt=len(txe), Br=wr.shape[0], Bt=wt.shape[0], T=1, L=L,
                   unblocked_records=unblocked, beam_taps_ms=statistics.median(ms_a), beam_taps_ms_all=ms_a,
                   array_taps_refused=refused, finite=bool(torch.isfinite(torch.view_as_real(out_a)).all()),
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
    if not all(r.get("faster", True) for r in rows):
        sys.exit("beam_taps is not faster than array_taps followed by the contraction")


if __name__ == "__main__":
    main()
