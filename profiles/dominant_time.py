"""What the K strongest paths per link cost: Tracer.dominant_paths at K = 64 and K = 1024 on C3 (or any workload)
against two yardsticks measured in the same process, the two-level planted worst case, and the drop-in call.

    python profiles/dominant_time.py [--configs c3] [--reps 5] [--out profiles/dominant/dominant_time_c3.json]

In ONE process, per config: a Tracer traces the whole launch set once; then, each timed with HIP events around each of
`reps` calls (median reported):
    dominant_paths(K)            the selection, K = 64 and K = 1024
    power_profiles, moments only yardstick (a): Ld = 0 and no spectra, the cheapest sibling pass over every record
and, as wall time around a synchronised call,
    paths() + torch.topk         yardstick (b), the only route there was: the full list, then a top K per link on the
                                 device (--no-topk skips it).
--worst adds the planted worst case: the `room` configuration of the tests (two TX, > 1 024 triangles) with
tests/planted.py's two power levels per link, where the tie-break is the whole comparison.  --no-drop-in skips the
warm hermespy_rt.compute_dominant_paths / compute_paths comparison.
Kernel times by rocprof: run this with --no-drop-in --no-topk under `rocprofv3 --kernel-trace --stats -d <dir> --
python ...`."""
import argparse
import json
import os
import statistics
import sys
import tempfile
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

KS = (64, 1024)


def drop_in_args(c):
    return (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], len(c["rx_pos"]),
            len(c["tx_pos"]), c["num_paths"], c["num_bounces"])


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def event_ms(fn, reps):
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
    return statistics.median(ms), ms


def topk_route(tr, k):
    """the route without the feature: the full list, then the k strongest of every link (power only: the tie-break
    and the gather of the other fields would come on top)"""
    P = tr.paths(nonzero_only=True)
    a, b = torch.view_as_real(P["a_te"]).double(), torch.view_as_real(P["a_tm"]).double()
    power = (a * a).sum(-1) + (b * b).sum(-1)
    link = P["rx"] * tr.ntx + P["tx"]
    out = []
    for lk in range(tr.nrx * tr.ntx):
        p = power[link == lk]
        out.append(torch.topk(p, min(k, p.numel())))
    return out


def device_row(tr, reps, topk):
    row = dict(links=tr.nrx * tr.ntx, records=int(tr.work()["records"]))
    row["unblocked"] = int(tr.paths(nonzero_only=False)["unblocked"].sum().item())
    row["power_moments_ms"], row["power_moments_ms_all"] = event_ms(lambda: tr.power_profiles(0.0, 1e-8, 0), reps)
    for k in KS:
        out = tr.dominant_paths(k)["buffer"]
        row["dominant_%d_ms" % k], row["dominant_%d_ms_all" % k] = event_ms(lambda: tr.dominant_paths(k, out=out),
                                                                           reps)
        row["dominant_%d_over_moments" % k] = row["dominant_%d_ms" % k] / row["power_moments_ms"]
        if topk:
            wall(lambda: topk_route(tr, k))
            t = [wall(lambda: topk_route(tr, k))[0] * 1e3 for _ in range(max(reps // 2, 2))]
            row["paths_topk_%d_ms" % k], row["paths_topk_%d_ms_all" % k] = statistics.median(t), t
            row["paths_topk_%d_over_dominant" % k] = row["paths_topk_%d_ms" % k] / row["dominant_%d_ms" % k]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-drop-in", action="store_true", help="device times only")
    ap.add_argument("--no-topk", action="store_true", help="skip the paths() + topk yardstick")
    ap.add_argument("--worst", action="store_true", help="add the planted two-level worst case on the room scene")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name in [n for n in a.configs.split(",") if n]:
        c = W.WORKLOADS[name]
        args = drop_in_args(c)
        row = dict(config=name)
        if not a.no_drop_in:
            for k in KS:
                dm = lambda: hermespy_rt.compute_dominant_paths(*args, k)  # noqa: E731
                dp = lambda: hermespy_rt.compute_paths(*args)  # noqa: E731
                dm()
                dp()
                tm, td = [], []
                for _ in range(a.reps):
                    tm.append(wall(dm)[0])
                    td.append(wall(dp)[0])
                row.update({"compute_dominant_paths_%d_s" % k: statistics.median(tm),
                            "compute_dominant_paths_%d_all_s" % k: tm, "compute_paths_s": statistics.median(td),
                            "compute_paths_all_s": td})
                row["ratio_%d" % k] = row["compute_dominant_paths_%d_s" % k] / row["compute_paths_s"]
            hermespy_rt.cache_clear()
        tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"],
                    c["num_paths"], c["num_bounces"])
        tr.trace()
        row.update(device_row(tr, a.reps, not a.no_topk))
        tr.close()
        del tr
        torch.cuda.empty_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.worst:
        from tests import planted as PL
        from tests import scenes_gen as G
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "room.hrt")
            G.room_with_clutter(p, 120, seed=5)
            c = G.cfg(p, [[3.0, 2.0, 1.5], [-5.0, 4.0, 2.0]], [[-10.0, -6.0, 3.0], [12.0, 5.0, 4.0]], 6000, 3,
                      tx_vel=[[1.0, 0.0, 0.0], [0.0, -2.0, 0.0]])
            tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"],
                        c["num_paths"], c["num_bounces"])
            tr.trace()
            before = device_row(tr, a.reps, False)
            T = PL.plant(tr)
            row = dict(config="room_planted", traced=before, terms=int(T["rx"].size), **device_row(tr, a.reps, False))
            tr.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
