"""What per-link power statistics cost: hermespy_rt.compute_power_profiles against hermespy_rt.compute_paths, and the
power kernels' device time, on C3 (or any workload) with Ld = 1 024 delay bins of 10 ns and both angular spectra at
Nth x Nph = 32 x 64.

    python profiles/power_time.py [--configs c3] [--reps 5] [--out profiles/power/power_time_c3.json]

In ONE process, per config: after a warm-up call of each, the two drop-in calls alternate (`reps` times each) and the
median wall times are reported (--no-drop-in skips them); then a Tracer traces the whole launch set once and a whole
hrt_power_profiles call is timed with HIP events around each of `reps` calls.  Bytes: 44 per unblocked record per
pass (amplitudes, tau, direction, DFS, the ray id and FS0), two passes (moments, histograms), over kernel time.
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

BYTES_PER_RECORD = 44
SPEC = dict(tau0=0.0, dtau=1e-8, num_delay_bins=1024, num_zenith_bins=32, num_azimuth_bins=64)


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-drop-in", action="store_true", help="device times only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.configs.split(","):
        c = W.WORKLOADS[name]
        args = drop_in_args(c)
        row = dict(config=name, **SPEC)
        if not a.no_drop_in:
            pp = lambda: hermespy_rt.compute_power_profiles(*args, **SPEC)  # noqa: E731
            dp = lambda: hermespy_rt.compute_paths(*args)  # noqa: E731
            pp()
            dp()
            tp, td = [], []
            for _ in range(a.reps):
                tp.append(wall(pp)[0])
                td.append(wall(dp)[0])
            row.update(compute_power_profiles_s=statistics.median(tp), compute_power_profiles_all_s=tp,
                       compute_paths_s=statistics.median(td), compute_paths_all_s=td)
            row["ratio"] = row["compute_power_profiles_s"] / row["compute_paths_s"]
            hermespy_rt.cache_clear()
        tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"],
                    c["num_paths"], c["num_bounces"])
        tr.trace()
        records = int(tr.work()["records"])
        unblocked = int(tr.paths(nonzero_only=False)["unblocked"].sum().item())
        out = tr.power_profiles(**SPEC)["buffer"]
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.power_profiles(**SPEC, out=out)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        nbytes = 2.0 * BYTES_PER_RECORD * unblocked
        row.update(links=tr.nrx * tr.ntx, records=records, unblocked=unblocked, call_ms=statistics.median(ms),
                   call_ms_all=ms, bytes=nbytes, tb_per_s=nbytes / (statistics.median(ms) * 1e-3) / 1e12)
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
