"""expf's 2^(i/32) table on the device: the kernels read a copy of hrt_exp2_tab (csrc/hrt_libm.h) that they stage into
LDS, so a wrong word, a wrong place in the LDS image or a missing barrier shows as a wrong exponential.  Both users of
the table are evaluated ON THE GPU through hrt_selftest_math -- expf itself (fn 2) and scatter_pattern (fn 10), which
is what the record kernels call -- on inputs that reach every entry of the table (tests/test_exp_table_design.py),
with the float neighbours of 0 and -4 pi, and must equal a HOST build of the same header bit for bit."""
import numpy as np
import pytest

from tests import exp_table_util as U
from tests.test_gpu_libm import _device_eval

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_expf_reads_every_table_entry(product_lib, tmp_path):
    H = U.host_build(tmp_path)
    x = np.concatenate([U.table_inputs(), U.edge_inputs()])
    assert set(U.host_index(H, U.table_inputs()).tolist()) == set(range(32))
    got, want = _device_eval(product_lib, 2, x), U.host_expf(H, x)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, "%d of %d differ, e.g. x=%r (table entry %d): device 0x%08x host 0x%08x" % (
        bad.size, x.size, x[bad[0]], U.host_index(H, x[bad[:1]])[0], _bits(got)[bad[0]], _bits(want)[bad[0]])


def test_scatter_pattern_reads_every_table_entry(product_lib, tmp_path):
    H = U.host_build(tmp_path)
    items = U.scatter_items(np.concatenate([U.table_inputs(), U.edge_inputs()]))
    # (more than one workgroup of the selftest kernel, each with a table of its own, and a partial last wave)
    assert items.shape[0] > 4 * 256 and items.shape[0] % 64 != 0
    got = _device_eval(product_lib, 10, items.reshape(-1)).reshape(-1, 4)
    want = U.host_scatter(H, items)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, "%d values differ, e.g. item %d (s, alpha, th_s, th_i) = %s: device %s host %s" % (
        len(bad), bad[0][0], items[bad[0][0]], got[bad[0][0]], want[bad[0][0]])
    assert np.abs(want).max() > 0.1   # (the pattern is not zero: s > 0 on every item)
