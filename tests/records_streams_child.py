"""One case of tests/test_gpu_records_streams.py in a process of its own (HRT_TUNE is read once per problem, HRT_OVERLAP
by every trace; the parent test sets them): `python -m tests.records_streams_child <case>` runs the product and the
oracle on the case and compares bit for bit; prints STREAMS_OK on success."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import oracle  # noqa: E402
from tests import configs as K  # noqa: E402
from tests.parity import assert_bit_equal  # noqa: E402
from tests.records_occupancy_child import dense  # noqa: E402
from tests.test_gpu_records_streams import case_config  # noqa: E402

POISON = 0x7FC0DEAD   # a quiet NaN with a payload no kernel writes
REPEATS = 5


def back_to_back(c, ref):
    """The device-resident tracer on a stream of its own: record and mask blocks poisoned, one trace, everything kept;
    then REPEATS times (poison, trace) with no synchronisation in between, ONLY the caller's stream synchronised, and
    every word of every record and mask block must be the first trace's -- the last trace's records kernels, on the
    records streams, are behind the join; the poison and the memset of a later repeat are behind the records kernels of
    the one before."""
    import torch
    from hermespy_rt_amd.abi import written
    from hermespy_rt_amd.device import Tracer
    nb = c["num_bounces"]
    caller = torch.cuda.Stream()
    with torch.cuda.stream(caller):
        tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"], c["num_paths"], nb)

        def poison():
            for b in range(nb):
                tr.rec_block(b).fill_(POISON)
                tr.mask_block(b).fill_(POISON)

        def blocks():
            return [(tr.rec_block(b).cpu().numpy().copy(), tr.mask_block(b).cpu().numpy().copy()) for b in range(nb)]

        poison()
        tr.trace()
        torch.cuda.synchronize()
        first = blocks()
        live = [int(x) for x in tr.counts()[:nb + 1]]
        assert live == [int(x) for x in ref["extras"]["live"]], live
        # the first trace is the oracle's, bit for bit (so "equal to the first" below means "right")
        d = tr.to_dense()
        s = ref["scat"]
        assert np.array_equal(written(d["a_te_re"]), written(s["a_te_re"]))
        for k in ("a_te_re", "a_te_im", "a_tm_re", "a_tm_im", "tau", "directions_rx"):
            assert_bit_equal(d[k], s[k], k)
        assert all((r != POISON).any() and (m != POISON).any() for r, m in first)
        torch.cuda.synchronize()
        for _ in range(REPEATS):
            poison()
            tr.trace()
        caller.synchronize()   # the caller's stream alone
        again = blocks()
        bad = [(b, int((r0 != r1).sum()), int((m0 != m1).sum())) for b, ((r0, m0), (r1, m1)) in enumerate(zip(first, again))
               if not (np.array_equal(r0, r1) and np.array_equal(m0, m1))]
        assert not bad, "blocks that differ from the first trace's (bounce, record words, mask words): %s" % bad
        torch.cuda.synchronize()
        tr.close()
    return {"live": live}


def main():
    name = sys.argv[1]
    c, kind = case_config(name)
    ref = oracle.compute_paths(*K.args(c))
    out = (back_to_back if kind == "back_to_back" else dense)(c, ref)
    print(name, [int(x) for x in ref["extras"]["live"]], out, flush=True)
    print("STREAMS_OK", name)


if __name__ == "__main__":
    main()
