#!/usr/bin/env python3
"""Per-launch duration of a kernel from `rocprofv3 --kernel-trace` csv files:
    python profiles/trace_launch_medians.py KERNEL_SUBSTRING RUN_DIR [RUN_DIR ...]
For every run directory (searched for *kernel_trace.csv) the dispatches whose name holds the substring are dealt round
robin to the launches of a step (the dispatch order within a step repeats) and the median, minimum and maximum duration of
each launch are printed in microseconds, with the sum of the medians."""
import csv
import glob
import os
import statistics
import sys


def launches_per_step(rows, all_rows):
    """dispatches of the kernel between two dispatches of the step's first kernel (hrt_fused_kernel: launch 0)"""
    firsts = [i for i, r in enumerate(all_rows) if "hrt_fused_kernel" in r["Kernel_Name"]]
    if len(firsts) < 2:
        return 1
    ids = {id(r) for r in rows}
    return max(1, sum(1 for r in all_rows[firsts[-2]:firsts[-1]] if id(r) in ids))


def main():
    sub = sys.argv[1]
    for d in sys.argv[2:]:
        f = max(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
        all_rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
        rows = [r for r in all_rows if sub in r["Kernel_Name"]]
        if not rows:
            print("%s: no dispatch of a kernel named *%s*" % (d, sub))
            continue
        n = launches_per_step(rows, all_rows)
        names = sorted({r["Kernel_Name"][r["Kernel_Name"].find("hrt_"):].split("(")[0] for r in rows})
        med = []
        print("%s: %d dispatches, %d per step, %s" % (d, len(rows), n, "; ".join(names)))
        for k in range(n):
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[k::n]]
            med.append(statistics.median(us))
            print("  launch slot %d: median %.1f us (%.1f ... %.1f), %d calls" % (k, med[-1], min(us), max(us), len(us)))
        print("  sum of medians %.1f us" % sum(med))


if __name__ == "__main__":
    main()
