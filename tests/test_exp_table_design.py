"""No GPU: the inputs of tests/test_gpu_exp_table.py reach every entry of expf's 2^(i/32) table (csrc/hrt_libm.h), as
the header itself -- compiled for the host -- indexes it, and the header's expf equals the host libm's on them."""
import numpy as np

from oracle import oracle
from tests import exp_table_util as U


def test_the_inputs_reach_all_32_table_entries(tmp_path):
    H = U.host_build(tmp_path)
    x = U.table_inputs()
    assert x.size == U.K_MAX + 1 and (x < 0).all() and x.min() > -4.0 * np.pi
    idx = U.host_index(H, x)
    hit = np.bincount(idx, minlength=32)
    # (an input lies half a table step from both neighbouring entries: which of the two it reaches is the rounding of
    # its float, so the 18 rounds do not reach every entry 18 times -- but every entry is reached)
    assert hit.shape == (32,) and (hit > 0).all(), hit
    # the exponents a scatter item carries are these x exactly
    xs = np.concatenate([x, U.edge_inputs()])
    items = U.scatter_items(xs)
    big = xs[np.abs(xs) > 1e-30]
    want = np.concatenate([xs, big, big])
    got = -items[:, 1] * np.abs(items[:, 2] - items[:, 3])
    assert np.array_equal(got.view(np.uint32) & 0x7fffffff, want.view(np.uint32) & 0x7fffffff)


def test_the_host_build_equals_the_host_libm_on_them(tmp_path):
    H = U.host_build(tmp_path)
    x = np.concatenate([U.table_inputs(), U.edge_inputs()])
    got, ref = U.host_expf(H, x), oracle.host_libm("expf", x)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
