"""What impulse responses (taps) cost: hermespy_rt.compute_taps against hermespy_rt.compute_paths, and the taps
kernels' device time, on C3 in two shapes: T = 1, L = 256 at f_s = 122.88 MHz, and the shape a time-domain simulator
asks for, T = 1 024 samples at dt = 1 / f_s, L = 64.

    python profiles/taps_time.py [--configs c3] [--reps 3] [--out profiles/taps/taps_time_c3.json]

In ONE process, per config and shape: after a warm-up call of each, the two drop-in calls alternate (`reps` times
each) and the median wall times are reported (--no-drop-in skips them); then a Tracer traces the whole launch set
once and the taps kernels (hrt_taps) are timed with HIP events around `reps` calls.  Achieved FLOP: 8 * T * L per
unblocked record (2 polarisations x re, im x multiply-add) over kernel time, as a share of the FP32 peak (157.3 TF).
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
FS = 122.88e6
# (name, T, L, dt)
SHAPES = [("t1_l256", 1, 256, 0.0), ("t1024_l64", 1024, 64, 1.0 / FS)]


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
    ap.add_argument("--configs", default="c3")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-drop-in", action="store_true", help="device times only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.configs.split(","):
        c = W.WORKLOADS[name]
        args = drop_in_args(c)
        for shape, T, L, dt in SHAPES:
            if shape not in a.shapes.split(","):
                continue
            row = dict(config=name, shape=shape, T=T, L=L, fs=FS, dt=dt)
            if not a.no_drop_in:
                tp = lambda: hermespy_rt.compute_taps(*args, FS, L, dt=dt, num_times=T)  # noqa: E731
                dp = lambda: hermespy_rt.compute_paths(*args)  # noqa: E731
                tp()
                dp()
                tt, td = [], []
                for _ in range(a.reps):
                    tt.append(wall(tp)[0])
                    td.append(wall(dp)[0])
                row.update(compute_taps_s=statistics.median(tt), compute_taps_all_s=tt,
                           compute_paths_s=statistics.median(td), compute_paths_all_s=td)
                row["ratio"] = row["compute_taps_s"] / row["compute_paths_s"]
                hermespy_rt.cache_clear()
            tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"],
                        c["num_paths"], c["num_bounces"])
            tr.trace()
            records = int(tr.work()["records"])
            unblocked = int(tr.paths(nonzero_only=False)["unblocked"].sum().item())
            out = tr.taps(FS, L, dt=dt, num_times=T)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tr.taps(FS, L, dt=dt, num_times=T, out=out)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            flop = 8.0 * unblocked * T * L
            row.update(records=records, unblocked=unblocked, kernel_ms=statistics.median(ms), kernel_ms_all=ms,
                       flop=flop, tflops=flop / (statistics.median(ms) * 1e-3) / 1e12,
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
