"""The timeline of one median step out of a `rocprofv3 --kernel-trace --output-format csv` run of a plain
`python bench.py --workload c3 --steps 20 --warmup 5` (records streams on, no counters in the run):

    python profiles/streams/timeline.py <kernel_trace.csv> <out.json> ["what was run"]

A step begins with launch 0's kernel (hrt_fused_kernel) and ends with the last kernel before the next one.  Of all
steps with the full set of kernels, the one of median length is written out: start and end of every kernel in us from
the step's start, the stream it ran on, when the bounce chain (every kernel but hrt_records_kernel) ends, when each
records kernel starts, and the stretch at the end in which only records kernels run."""
import csv
import json
import re
import sys


def short(name):
    m = re.search(r"(hrt_\w+(?:<[^>]*>)?)", name)
    return m.group(1) if m else name[:40]


def main():
    path, out = sys.argv[1], sys.argv[2]
    rows = [r for r in csv.DictReader(open(path)) if "hrt_" in r["Kernel_Name"] and "build" not in r["Kernel_Name"]
            and "pencil" not in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    steps, cur = [], None
    for r in rows:
        if "hrt_fused_kernel" in r["Kernel_Name"]:
            cur = []
            steps.append(cur)
        if cur is not None:
            cur.append(r)
    full = max(len(s) for s in steps)
    steps = [s for s in steps if len(s) == full]
    span = lambda s: max(int(r["End_Timestamp"]) for r in s) - int(s[0]["Start_Timestamp"])
    steps.sort(key=span)
    s = steps[len(steps) // 2]
    t0 = int(s[0]["Start_Timestamp"])
    us = lambda t: round((int(t) - t0) / 1000.0, 2)
    kernels = [{"kernel": short(r["Kernel_Name"]), "stream": int(r["Stream_Id"]), "queue": int(r["Queue_Id"]),
                "start_us": us(r["Start_Timestamp"]), "end_us": us(r["End_Timestamp"]),
                "us": round((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0, 2)} for r in s]
    rec = [k for k in kernels if k["kernel"].startswith("hrt_records_kernel")]
    chain = [k for k in kernels if not k["kernel"].startswith("hrt_records_kernel")]
    chain_end = max(k["end_us"] for k in chain)
    step_end = max(k["end_us"] for k in kernels)
    # how many records kernels run at a time, in us of the step
    edges = sorted([(k["start_us"], 1) for k in rec] + [(k["end_us"], -1) for k in rec])
    depth, last, by_depth = 0, 0.0, {}
    for t, d in edges:
        by_depth[depth] = round(by_depth.get(depth, 0.0) + t - last, 2)
        depth, last = depth + d, t
    res = {
        "what": sys.argv[3] if len(sys.argv) > 3 else path,
        "steps_in_trace": len(steps),
        "step_us_min_median_max": [round(span(steps[0]) / 1000.0, 2), round(span(s) / 1000.0, 2),
                                   round(span(steps[-1]) / 1000.0, 2)],
        "kernels": kernels,
        "bounce_chain_ends_us": chain_end,
        "bounce_chain_work_us": round(sum(k["us"] for k in chain), 2),
        "records_start_us": [k["start_us"] for k in rec],
        "records_end_us": [k["end_us"] for k in rec],
        "records_us": [k["us"] for k in rec],
        "records_only_tail_us": round(step_end - chain_end, 2),
        "us_with_n_records_kernels_running": {str(k): v for k, v in sorted(by_depth.items())},
        "step_end_us": step_end,
    }
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "kernels"}, indent=1))


if __name__ == "__main__":
    main()
