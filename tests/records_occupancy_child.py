"""One case of tests/test_gpu_records_occupancy.py in a process of its own (HRT_OVERLAP and the tables' staging are
latched per process): `python -m tests.records_occupancy_child <case> <tmp dir>` runs the product and the oracle on the
case and compares every output array bit for bit; prints RECORDS_OK on success."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import oracle  # noqa: E402
from tests import configs as K  # noqa: E402
from tests.parity import assert_bit_equal, compare_dense  # noqa: E402
from tests.test_gpu_records_occupancy import case_config  # noqa: E402


def dense(c, ref):
    """the drop-in entry: every dense array of the reference"""
    from hermespy_rt_amd import abi, lib
    got = abi.run_compute_paths(lib.load(), *K.args(c))
    st = compare_dense(got, ref)
    assert all(v == 0 for v in st.values()), st
    return st


def timer_pass(c, ref, records_kernel=True):
    """the device-resident entry with HIP events around every kernel (hrt_trace_flags with a timer); records_kernel:
    hrt_records_kernel runs on this problem, so its phase takes time"""
    from hermespy_rt_amd.abi import written
    from hermespy_rt_amd.device import Tracer
    tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"], c["num_paths"],
                c["num_bounces"])
    t = tr.new_timer()
    tr.trace_with_timer(t)
    times = tr.read_timer(t)
    assert len(times["records_ms"]) == c["num_bounces"] + 1 and (max(times["records_ms"]) > 0.0 or not records_kernel), times
    d = tr.to_dense()
    ex, s = ref["extras"], ref["scat"]
    assert list(d["counts"][:c["num_bounces"] + 1]) == [int(x) for x in ex["live"]]
    assert np.array_equal(d["hit_tri"], ex["hit_tri"])
    assert np.array_equal(written(d["a_te_re"]), written(s["a_te_re"]))
    for k in ("a_te_re", "a_te_im", "a_tm_re", "a_tm_im", "tau", "directions_rx"):
        assert_bit_equal(d[k], s[k], k)
    tr.close()
    return times


def main():
    name, tmp = sys.argv[1], sys.argv[2]
    c, kind = case_config(name, tmp)
    ref = oracle.compute_paths(*K.args(c))
    live = [int(x) for x in ref["extras"]["live"]]
    out = (timer_pass if kind == "timer" else dense)(c, ref)
    print(name, live, out, flush=True)
    print("RECORDS_OK", name)


if __name__ == "__main__":
    main()
