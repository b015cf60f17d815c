"""What antenna-array impulse responses cost: hermespy_rt.compute_array_taps against hermespy_rt.compute_array_channel
(K = 256, T = 1), and the array taps kernels' device time, on C3 with a 4-element RX ULA and a 4 x 4 TX UPA at lambda / 2
(64 element pairs), f_s = 122.88 MHz, f_c = f_a = the carrier, in two shapes: T = 1, L = 256, and T = 64, L = 64 at
dt = 1 / f_s.

    python profiles/array_taps_time.py [--configs c3] [--reps 5] [--out profiles/array_taps/array_taps_time_c3.json]

In ONE process, per config and shape: after a warm-up call of each, the drop-in calls compute_array_taps and
compute_array_channel alternate (`reps` times each) and the median wall times are reported (--no-drop-in skips them);
then a Tracer traces the whole launch set once and Tracer.array_taps (and, for comparison, Tracer.array_channel at
K = 256) are timed with HIP events around `reps` calls each.  Achieved FLOP: 8 * Nr * Nt * T * L per unblocked record
(2 polarisations x re, im x multiply-add) over the call's device time, as a share of the FP32 peak (157.3 TF).  Kernel
times by rocprof: run this under `rocprofv3 --kernel-trace --stats -d <dir> -- python ...`."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import hermespy_rt_amd  # noqa: E402
import torch  # noqa: E402,F401  (HIP runtime first, see hermespy_rt_amd.lib)

sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
import hermespy_rt  # noqa: E402

from hermespy_rt_amd import workloads as W  # noqa: E402
from hermespy_rt_amd.device import Tracer  # noqa: E402

PEAK_FP32 = 157.3e12
FS = 122.88e6
C0 = 299792458.0
K_CHANNEL, DF = 256, 30e3
# (name, T, L, dt)
SHAPES = [("t1_l256", 1, 256, 0.0), ("t64_l64", 64, 64, 1.0 / FS)]


def elements(f_ghz):
    """the RX ULA (4 along y) and the TX UPA (4 x 4 in x, z) at lambda / 2"""
    d = C0 / (f_ghz * 1e9) / 2
    rxe = np.zeros((4, 3), np.float32)
    rxe[:, 1] = np.arange(4) * d
    txe = np.zeros((16, 3), np.float32)
    txe[:, 0] = np.repeat(np.arange(4), 4) * d
    txe[:, 2] = np.tile(np.arange(4), 4) * d
    return rxe, txe


def drop_in_args(c):
    return (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], len(c["rx_pos"]),
            len(c["tx_pos"]), c["num_paths"], c["num_bounces"])


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def events(fn, reps):
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-drop-in", action="store_true", help="device times only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.configs.split(","):
        c = W.WORKLOADS[name]
        args = drop_in_args(c)
        rxe, txe = elements(c["f_ghz"])
        f0 = c["f_ghz"] * 1e9 - (K_CHANNEL // 2) * DF
        npairs = rxe.shape[0] * txe.shape[0]
        for shape, T, L, dt in SHAPES:
            if shape not in a.shapes.split(","):
                continue
            row = dict(config=name, shape=shape, T=T, L=L, fs=FS, dt=dt, nr=rxe.shape[0], nt=txe.shape[0])
            if not a.no_drop_in:
                at = lambda: hermespy_rt.compute_array_taps(*args, FS, L, rxe, txe, dt=dt, num_times=T)  # noqa: E731
                ac = lambda: hermespy_rt.compute_array_channel(*args, f0, DF, K_CHANNEL, rxe, txe)  # noqa: E731
                at()
                ac()
                ta, tc = [], []
                for _ in range(a.reps):
                    ta.append(wall(at)[0])
                    tc.append(wall(ac)[0])
                row.update(compute_array_taps_s=statistics.median(ta), compute_array_taps_all_s=ta,
                           compute_array_channel_k256_s=statistics.median(tc), compute_array_channel_k256_all_s=tc)
                row["ratio"] = row["compute_array_taps_s"] / row["compute_array_channel_k256_s"]
                hermespy_rt.cache_clear()
            tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"],
                        c["num_paths"], c["num_bounces"])
            tr.trace()
            records = int(tr.work()["records"])
            unblocked = int(tr.paths(nonzero_only=False)["unblocked"].sum().item())
            out = tr.array_taps(rxe, txe, FS, L, dt=dt, num_times=T)
            ch = tr.array_channel(rxe, txe, f0, DF, K_CHANNEL)
            torch.cuda.synchronize()
            ms = events(lambda: tr.array_taps(rxe, txe, FS, L, dt=dt, num_times=T, out=out), a.reps)
            ms_ch = events(lambda: tr.array_channel(rxe, txe, f0, DF, K_CHANNEL, out=ch), a.reps)
            flop = 8.0 * unblocked * npairs * T * L
            row.update(records=records, unblocked=unblocked, call_ms=statistics.median(ms), call_ms_all=ms,
                       array_channel_k256_call_ms=statistics.median(ms_ch), array_channel_k256_call_ms_all=ms_ch,
                       flop=flop, tflops=flop / (statistics.median(ms) * 1e-3) / 1e12,
                       peak_share=flop / (statistics.median(ms) * 1e-3) / PEAK_FP32)
            tr.close()
            del tr, out, ch
            torch.cuda.empty_cache()
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
