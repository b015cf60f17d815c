#!/usr/bin/env python3
"""The standing rule's rounds: plain `python bench.py --workload W` on two builds of the library side by side (the
parent's in one directory, the new one in another; HRT_LIB_DIR selects), in alternation, parent first, one process
per run, one card.
    python profiles/bench_rounds.py OUT.json PARENT_LIB_DIR NEW_LIB_DIR W:ROUNDS [W:ROUNDS ...]
Every run has a time limit; after a run that fails nothing more is started.  OUT.json: per workload the rounds of both
builds (ms per step), their medians and ranges, and whether the medians differ by twice the parent's range."""
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_TIMEOUT_S = 240


def one_run(lib_dir, workload):
    env = dict(os.environ, HRT_LIB_DIR=os.path.abspath(lib_dir))
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--workload", workload], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=RUN_TIMEOUT_S)
    if p.returncode != 0:
        sys.exit("bench.py --workload %s with %s: exit %d\n%s" % (workload, lib_dir, p.returncode, p.stderr[-2000:]))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def main():
    out_path, parent, new = sys.argv[1:4]
    result = {}
    for spec in sys.argv[4:]:
        w, rounds = spec.split(":")
        rows = {"parent": [], "new": [], "notes": []}
        for r in range(int(rounds)):
            for name, d in (("parent", parent), ("new", new)):
                res = one_run(d, w)
                rows[name].append(res["ms_per_step"])
                if res.get("fallback_state") or res.get("void_regions_retimed"):   # a kernel timed out on a shared card
                    rows["notes"].append("%s round %d: fallback_state %s, regions retimed %s" % (
                        name, r, res.get("fallback_state"), res.get("void_regions_retimed")))
                print(w, r, name, res["ms_per_step"], "ms per step", flush=True)
            result[w] = dict(rows)
            for name in ("parent", "new"):
                v = rows[name]
                result[w][name + "_median"] = statistics.median(v)
                result[w][name + "_range"] = max(v) - min(v)
            result[w]["parent_minus_new"] = result[w]["parent_median"] - result[w]["new_median"]
            result[w]["bar"] = 2.0 * result[w]["parent_range"]
            result[w]["new_median_above_parent_range"] = result[w]["new_median"] > max(rows["parent"])
            with open(out_path, "w") as f:   # (after every round: a later failure keeps what was measured)
                json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
