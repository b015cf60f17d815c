#!/usr/bin/env python3
"""Phase stamps of a fused launch's workgroups (library built with `make EXTRA=-DHRT_PHASE_STATS`; the stamps stand in
csrc/hrt_fused_body.inc, thread 0 of every workgroup, 100 MHz wall clock):
    HRT_LIB_DIR=<that build> python profiles/phase_stamps.py WORKLOAD OUT.json [LAUNCH]
traces the bench workload three times, has the library dump the stamps of the last trace (HRT_PHASE_FILE) and writes
per phase of a workgroup's life the median and the 10th and 90th percentile in microseconds, the life itself, the
launch's span (first start to last end) and how many workgroups were alive together, on average, over that span.  With
HRT_PHASE_FILE set such a build also prints what hipOccupancyMaxActiveBlocksPerMultiprocessor answers for the launch-0
instantiation at its real LDS size (stderr)."""
import ctypes
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
workload, out_path = sys.argv[1], sys.argv[2]
launch = int(sys.argv[3]) if len(sys.argv) > 3 else 0
raw = os.path.join(tempfile.mkdtemp(), "phase.bin")
os.environ["HRT_PHASE_FILE"] = raw
os.environ["HRT_PHASE_BOUNCE"] = str(launch)

import torch  # noqa: E402
from hermespy_rt_amd import lib  # noqa: E402
from hermespy_rt_amd.device import Tracer  # noqa: E402
from hermespy_rt_amd.workloads import WORKLOADS  # noqa: E402

w = WORKLOADS[workload]
tr = Tracer(w["scene_path"], w["rx_pos"], w["tx_pos"], w["rx_vel"], w["tx_vel"], w["f_ghz"], w["num_paths"], w["num_bounces"])
for _ in range(3):
    tr.trace()
    torch.cuda.synchronize()
err = int(tr.error_word())
arr = (ctypes.c_uint64 * 48)()
lib.load().hrt_debug_kernel_stats(0, arr, 0)
ph = np.fromfile(raw, np.uint64).reshape(65536, 8)
ph = ph[ph[:, 0] != 0][:, :6].astype(np.int64)
TICK_US = 0.01
names = ["loads_and_staging", "traces_and_publish", "records", "prefix_wait", "shade_and_stores"]


def pct(x):
    return dict(p10=round(float(np.percentile(x, 10)), 2), median=round(float(np.median(x)), 2),
                p90=round(float(np.percentile(x, 90)), 2))


res = dict(workload=workload, launch=launch, workgroups=int(ph.shape[0]), error_word=err, unit="us")
for k, n in enumerate(names):
    res[n] = pct((ph[:, k + 1] - ph[:, k]) * TICK_US)
life = (ph[:, 5] - ph[:, 0]) * TICK_US
res["life"] = pct(life)
span = float(ph[:, 5].max() - ph[:, 0].min()) * TICK_US
res["span_first_start_to_last_end"] = round(span, 2)
res["mean_workgroups_alive"] = round(float(life.sum()) / span, 1)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
