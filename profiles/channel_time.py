"""What a channel costs: hermespy_rt.compute_channel against hermespy_rt.compute_paths, and the channel
kernels' device time, on C3 / C4 / C5 with K = 1 024 subcarriers (30 kHz around the carrier), T in {1, 14}.

    python profiles/channel_time.py [--configs c3,c4,c5] [--reps 3] [--out profiles/channel/channel_time.json]

In ONE process, per config and T: after a warm-up call of each, the two drop-in calls alternate (`reps` times
each) and the median wall times are reported; then a Tracer traces the whole launch set once and the channel
kernels (hrt_channel) are timed with HIP events around `reps` calls.  Achieved FLOP: 8 * records read * K * T
(records read: every scatter record of the trace, blocked ones included) over kernel time, as a share of the
FP32 peak (157.3 TF).  C5's compute_paths fills 147 GB of host arrays: it is only called with --dense-c5.
Kernel times by rocprof: run this under `rocprofv3 --kernel-trace --stats -d <dir> -- python ...`."""
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
K, DF = 1024, 30e3


def drop_in_args(c):
    return (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], len(c["rx_pos"]),
            len(c["tx_pos"]), c["num_paths"], c["num_bounces"])


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c4,c5")
    ap.add_argument("--times", default="1,14")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dense-c5", action="store_true")
    ap.add_argument("--no-drop-in", action="store_true", help="device times only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.configs.split(","):
        c = W.WORKLOADS[name]
        f0 = c["f_ghz"] * 1e9 - (K // 2) * DF
        args = drop_in_args(c)
        for T in [int(x) for x in a.times.split(",")]:
            dt = 1e-3 if T > 1 else 0.0
            row = dict(config=name, K=K, T=T)
            dense = not a.no_drop_in and (name != "c5" or a.dense_c5)
            if not a.no_drop_in:
                ch = lambda: hermespy_rt.compute_channel(*args, f0, DF, K, 0.0, dt, T)  # noqa: E731
                dp = lambda: hermespy_rt.compute_paths(*args)  # noqa: E731
                ch()
                if dense:
                    dp()
                tc, tp = [], []
                for _ in range(a.reps):
                    tc.append(wall(ch)[0])
                    if dense:
                        tp.append(wall(dp)[0])
                row["compute_channel_s"] = statistics.median(tc)
                row["compute_channel_all_s"] = tc
                if dense:
                    row["compute_paths_s"] = statistics.median(tp)
                    row["compute_paths_all_s"] = tp
                    row["speedup"] = row["compute_paths_s"] / row["compute_channel_s"]
                hermespy_rt.cache_clear()
            tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"],
                        c["num_paths"], c["num_bounces"])
            tr.trace()
            records = int(tr.work()["records"])
            out = tr.channel(f0, DF, K, dt=dt, num_times=T)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tr.channel(f0, DF, K, dt=dt, num_times=T, out=out)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            flop = 8.0 * records * K * T
            row.update(records=records, kernel_ms=statistics.median(ms), kernel_ms_all=ms, flop=flop,
                       tflops=flop / (statistics.median(ms) * 1e-3) / 1e12,
                       peak_share=flop / (statistics.median(ms) * 1e-3) / PEAK_FP32)
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
