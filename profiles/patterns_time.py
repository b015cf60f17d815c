"""What the antenna patterns cost: the device time of hrt_apply_patterns on a traced workspace (C3 and C4 by default),
for the TR 38.901 element on both sides and for a 181 x 360 table on both sides, against a device-to-device copy.

    python profiles/patterns_time.py [--configs c3,c4] [--reps 3] [--out profiles/patterns/patterns_time.json]

In ONE process, per config: a Tracer traces the whole launch set; per pattern pair, after a warm-up, `reps` times: a
plain trace (so that every timed call weights freshly traced amplitudes), then HIP events around one
hrt_apply_patterns call on the same stream; the median is reported.  The bytes the kernels need: per unblocked record
the three direction floats and four loads and four stores of the amplitude fields (44 B), per hit the ray id and its
share of the mask words (8 B).  The yardstick, in the same process: one hipMemcpyAsync device-to-device copy (torch's
Tensor.copy_) of that many bytes, which itself reads and writes every one of them; `ratio` is the apply time over the
copy's.  `bound_ms` is bytes over the HBM peak (8 TB/s)."""
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

from hermespy_rt_amd import patterns as P  # noqa: E402
from hermespy_rt_amd import workloads as W  # noqa: E402
from hermespy_rt_amd.device import Tracer  # noqa: E402

HBM_PEAK = 8.0e12
BYTES_PER_RECORD, BYTES_PER_HIT = 44, 8


def measured_table(nz=181, na=360):
    """a smooth directive pattern on the finest grid the entry takes"""
    th = np.pi * np.arange(nz) / (nz - 1)
    ph = -np.pi + 2 * np.pi * np.arange(na) / na
    t, p = np.meshgrid(th, ph, indexing="ij")
    return (0.05 + np.sin(t) ** 2 * (0.6 + 0.4 * np.cos(p)) ** 2).astype(np.float32)


def orientations(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([P.rotation(*rng.uniform(-np.pi, np.pi, 3)) for _ in range(n)])


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("patterns_time.py needs a HIP device: a time is measured on the GPU or not at all")
    rows = []
    for name in a.configs.split(","):
        c = W.WORKLOADS[name]
        tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"], c["num_paths"],
                    c["num_bounces"], device_dirs=True)
        tr.trace()
        counts = tr.counts()
        hits = int(sum(int(counts[b + 1]) for b in range(tr.nb)))
        unblocked = 0
        for b in range(tr.nb):
            if int(counts[b + 1]):
                unblocked += int(tr.records(b, int(counts[b + 1]))["unblocked"].sum().item())
        nbytes = BYTES_PER_RECORD * unblocked + BYTES_PER_HIT * hits
        src = torch.empty(nbytes, dtype=torch.uint8, device=tr.device)
        dst = torch.empty_like(src)
        dst.copy_(src)
        torch.cuda.synchronize()
        copy_ms = [events(lambda: dst.copy_(src)) for _ in range(a.reps)]
        copy = statistics.median(copy_ms)
        del src, dst
        R_rx, R_tx = orientations(tr.nrx, 1), orientations(tr.ntx, 2)
        table = P.table(measured_table())
        for label, rx, tx in (("tr38901", P.tr38901(), P.tr38901()), ("table_181x360", table, table),
                              ("isotropic", P.isotropic(3.0), P.isotropic(-3.0))):
            ms = []
            for rep in range(a.reps + 1):   # (the first is the warm-up)
                tr.set_patterns()
                tr.trace()
                tr.set_patterns(rx, tx, R_rx, R_tx)
                torch.cuda.synchronize()
                ms.append(events(tr.apply_patterns))
            ms = ms[1:]
            t = statistics.median(ms)
            row = dict(config=name, patterns=label, links=tr.nrx * tr.ntx, hits=hits, unblocked=unblocked, bytes=nbytes,
                       apply_ms=t, apply_ms_all=ms, copy_ms=copy, copy_ms_all=copy_ms, ratio=t / copy,
                       bound_ms=nbytes / HBM_PEAK * 1e3, gb_per_s=nbytes / (t * 1e-3) / 1e9)
            rows.append(row)
            print(json.dumps(row), flush=True)
        tr.set_patterns()
        tr.close()
        del tr
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
