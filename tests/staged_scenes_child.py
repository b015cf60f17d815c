"""One case of tests/test_gpu_staged_scenes.py in a process of its own: `python -m tests.staged_scenes_child <case>
<tmp dir>` runs the product and the oracle on the case and compares every output array bit for bit; prints STAGED_OK
on success."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import oracle  # noqa: E402
from tests import configs as K  # noqa: E402
from tests.parity import compare_dense  # noqa: E402
from tests.test_gpu_staged_scenes import case_config  # noqa: E402


def main():
    name, tmp = sys.argv[1], sys.argv[2]
    c = case_config(name, tmp)
    ref = oracle.compute_paths(*K.args(c))
    live = [int(x) for x in ref["extras"]["live"]]
    from hermespy_rt_amd import abi, lib
    got = abi.run_compute_paths(lib.load(), *K.args(c))
    st = compare_dense(got, ref)
    print(name, live, st, flush=True)
    assert all(v == 0 for v in st.values()), st
    print("STAGED_OK", name)


if __name__ == "__main__":
    main()
