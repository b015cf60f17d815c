"""What an antenna-array channel costs: hermespy_rt.compute_array_channel next to hermespy_rt.compute_channel, and
the array kernels' device time, on C3 with a 4-element RX ULA x 4 x 4 TX UPA at half a wavelength (64 element
pairs), K in {1 024, 256} subcarriers (30 kHz around the carrier), T in {1, 14}.

    python profiles/array_channel_time.py [--configs c3] [--ks 1024,256] [--times 1,14] [--reps 3]
                                          [--out profiles/array_channel/array_channel_time.json]

In ONE process, per config, K and T: after a warm-up call of each, the two drop-in calls alternate (`reps` times
each) and the median wall times are reported; then a Tracer traces the whole launch set once and the array kernels
(hrt_array_channel) are timed with HIP events around `reps` calls.  Achieved FLOP: 16 * unblocked scatter records *
Nr * Nt * T * K (two polarisations, 8 real flops per complex multiply-add; DESIGN section 10 counts 8 per record
and grid point, i.e. half of this per polarisation term) over kernel time, as a share of the FP32 MFMA peak
(157.3 TF).  Kernel times by rocprof: run this under `rocprofv3 --kernel-trace --stats -d <dir> -- python ...`."""
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
DF = 30e3
C0 = 299792458.0


def drop_in_args(c):
    return (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], len(c["rx_pos"]),
            len(c["tx_pos"]), c["num_paths"], c["num_bounces"])


def arrays(c):
    """4-element RX ULA along y, 4 x 4 TX UPA in the x-z plane, both at half a wavelength"""
    d = C0 / (c["f_ghz"] * 1e9) / 2
    rx = np.zeros((4, 3), np.float32)
    rx[:, 1] = np.arange(4) * d
    tx = np.zeros((16, 3), np.float32)
    tx[:, 0] = np.repeat(np.arange(4), 4) * d
    tx[:, 2] = np.tile(np.arange(4), 4) * d
    return rx, tx


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def unblocked_records(tr):
    counts = tr.counts()
    return sum(int(tr.records(b, int(counts[b + 1]))["unblocked"].sum().item())
               for b in range(tr.nb) if int(counts[b + 1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3")
    ap.add_argument("--ks", default="1024,256")
    ap.add_argument("--times", default="1,14")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-drop-in", action="store_true", help="device times only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.configs.split(","):
        c = W.WORKLOADS[name]
        rxe, txe = arrays(c)
        args = drop_in_args(c)
        for K in [int(x) for x in a.ks.split(",")]:
            f0 = c["f_ghz"] * 1e9 - (K // 2) * DF
            for T in [int(x) for x in a.times.split(",")]:
                dt = 1e-3 if T > 1 else 0.0
                row = dict(config=name, Nr=len(rxe), Nt=len(txe), K=K, T=T)
                if not a.no_drop_in:
                    ac = lambda: hermespy_rt.compute_array_channel(*args, f0, DF, K, rxe, txe, 0.0, dt, T)  # noqa: E731
                    ch = lambda: hermespy_rt.compute_channel(*args, f0, DF, K, 0.0, dt, T)  # noqa: E731
                    ac()
                    ch()
                    ta, tc = [], []
                    for _ in range(a.reps):
                        ta.append(wall(ac)[0])
                        tc.append(wall(ch)[0])
                    row.update(compute_array_channel_s=statistics.median(ta), compute_array_channel_all_s=ta,
                               compute_channel_s=statistics.median(tc), compute_channel_all_s=tc,
                               ratio=statistics.median(ta) / statistics.median(tc))
                    hermespy_rt.cache_clear()
                tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"],
                            c["num_paths"], c["num_bounces"])
                tr.trace()
                records = int(tr.work()["records"])
                unblocked = unblocked_records(tr)
                out = tr.array_channel(rxe, txe, f0, DF, K, dt=dt, num_times=T)
                torch.cuda.synchronize()
                ms = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    tr.array_channel(rxe, txe, f0, DF, K, dt=dt, num_times=T, out=out)
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                flop = 16.0 * unblocked * len(rxe) * len(txe) * K * T
                t = statistics.median(ms) * 1e-3
                row.update(records=records, unblocked_records=unblocked, kernel_ms=statistics.median(ms),
                           kernel_ms_all=ms, flop=flop, tflops=flop / t / 1e12, peak_share=flop / t / PEAK_FP32)
                tr.close()
                del tr, out
                torch.cuda.empty_cache()
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
