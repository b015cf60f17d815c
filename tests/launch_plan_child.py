"""One case of tests/test_gpu_launch_plan.py in a process of its own (HRT_TUNE is read per problem, the tables' staging
is latched per process): `python -m tests.launch_plan_child <records kernel expected: 0 | 1>` runs both passes of
tests/records_occupancy_child.py -- the drop-in entry against the oracle, every dense array bit for bit, and the
device-resident entry with a timer -- on the street canyon at 20 000 rays per TX, and prints the timer's phases as
one JSON line behind PLAN_TIMES."""
import json
import sys

from oracle import oracle
from tests import configs as K
from tests.records_occupancy_child import dense, timer_pass


def main():
    records_kernel = sys.argv[1] == "1"
    c = K.small(K.C3, 20000)
    ref = oracle.compute_paths(*K.args(c))
    print("dense", dense(c, ref), flush=True)
    times = timer_pass(c, ref, records_kernel=records_kernel)
    print("PLAN_TIMES " + json.dumps(times), flush=True)
    print("PLAN_OK")


if __name__ == "__main__":
    main()
