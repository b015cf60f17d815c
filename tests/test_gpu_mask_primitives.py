"""The primitives the patch-mask and record kernels were trimmed with (csrc/hrt_kernels.hip), each evaluated ON THE
GPU on arrays through hrt_selftest_math (fn 8 .. 10, include/hrt_device.h) and held against the host:

  * wave_or256 -- the union of eight mask words over a wave by half-wave and row swaps and four DPP steps -- against
    numpy's OR over each wave of 64 items, on random, all-zero, single-bit and single-lane inputs, whole waves and a
    partial last one;
  * div_c -- a / c in three instructions -- against the IEEE division on a strided sweep of [2^-60, 2^40) and on 0
    (tests/test_division_by_c.py compares the same sequence on EVERY float of the range on the host);
  * scatter_pattern, which the trimming left as it was, against the values recorded from it on an MI355X
    (tests/golden/scatter_pattern_grid.npy) on a grid of all 17 materials x 16 theta_s x 16 theta_i: the anchor for
    any later cut of its divisions.

Every GPU step is a process of its own under a time limit; after a step that failed, none is started again."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "scatter_pattern_grid.npy")
STEP_TIMEOUT_S = 120

_CHILD = """
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from hermespy_rt_amd import lib
L = lib.load()
x = np.ascontiguousarray(np.load(sys.argv[2]))
out = np.zeros_like(x)
f32p = C.POINTER(C.c_float)
lib.check(L.hrt_selftest_math(0, int(sys.argv[1]), x.ctypes.data_as(f32p), out.ctypes.data_as(f32p), x.size),
          "hrt_selftest_math")
np.save(sys.argv[3], out)
""" % REPO

_failed = []   # the first GPU step that failed: nothing is started after it


def device_eval(tmp_path, fn, x):
    """hrt_selftest_math(fn) over the float32 array x in a process of its own (bits in, bits out)."""
    if _failed:
        pytest.fail("not started: GPU step %s failed before" % _failed[0])
    x = np.ascontiguousarray(x, np.float32)
    src, dst = str(tmp_path / ("in%d.npy" % fn)), str(tmp_path / ("out%d.npy" % fn))
    np.save(src, x)
    try:
        p = subprocess.run([sys.executable, "-c", _CHILD, str(fn), src, dst], capture_output=True, text=True,
                           timeout=STEP_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _failed.append("fn %d (time limit)" % fn)
        raise
    if p.returncode != 0:
        _failed.append("fn %d (exit %d)" % (fn, p.returncode))
        pytest.fail("fn %d: exit %d\n%s" % (fn, p.returncode, p.stderr[-2000:]))
    out = np.load(dst)
    assert out.shape == x.shape and out.dtype == np.float32
    return out


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_wave_union(tmp_path):
    rng = np.random.default_rng(11)
    lanes = 64 * 5 + 17   # whole waves and a partial last one (its other lanes bring zeros)
    cases = {}
    cases["random"] = rng.integers(0, 2**32, (lanes, 8), dtype=np.uint64).astype(np.uint32)
    cases["sparse"] = (np.uint32(1) << rng.integers(0, 32, (lanes, 8)).astype(np.uint32)) * (rng.random((lanes, 8)) < 0.1)
    cases["zero"] = np.zeros((lanes, 8), np.uint32)
    one_bit = np.zeros((lanes, 8), np.uint32)   # one bit in the whole wave: every (lane, word) position in turn
    one_lane = np.zeros((lanes, 8), np.uint32)  # one lane of the wave carries all of it
    for wv in range((lanes + 63) // 64):
        lane = min(wv * 64 + (wv * 13 + 5) % 64, lanes - 1)
        one_bit[lane, wv % 8] = np.uint32(1) << np.uint32((7 * wv + 3) % 32)
        one_lane[lane] = rng.integers(1, 2**32, 8, dtype=np.uint64).astype(np.uint32)
    cases["one_bit"], cases["one_lane"] = one_bit, one_lane
    # every lane position alone, word k = lane % 8: 64 waves of 64 lanes
    sweep = np.zeros((64 * 64, 8), np.uint32)
    for lane in range(64):
        sweep[lane * 64 + lane, lane % 8] = np.uint32(0x80000001) + np.uint32(lane)
    cases["each_lane"] = sweep
    names = list(cases)
    sizes = [cases[k].shape[0] for k in names]
    pad = [(-s) % 64 for s in sizes]   # every case starts on a wave boundary
    words = np.concatenate([np.concatenate([cases[k].astype(np.uint32), np.zeros((p, 8), np.uint32)])
                            for k, p in zip(names, pad)])
    # the trailing padding of the LAST case is cut off again: its last wave is partial on the device
    words = words[:words.shape[0] - pad[-1]] if pad[-1] else words
    got = device_eval(tmp_path, 8, words.reshape(-1).view(np.float32)).view(np.uint32).reshape(-1, 8)
    full = np.concatenate([words, np.zeros(((-words.shape[0]) % 64, 8), np.uint32)])
    want = np.repeat(np.bitwise_or.reduce(full.reshape(-1, 64, 8), axis=1), 64, axis=0)[:words.shape[0]]
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%d words differ, first (lane, word) %s: got 0x%08x want 0x%08x" % (
        len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    assert want.any() and not want[sum(sizes[:2]) + sum(pad[:2]):sum(sizes[:3]) + sum(pad[:2])].any()


def test_division_by_c(tmp_path):
    lo, hi = int(bits(np.float32(2.0 ** -60))[0]), int(bits(np.float32(2.0 ** 40))[0])
    u = np.arange(lo, hi, 401, dtype=np.uint64).astype(np.uint32)   # 2.09e6 of the 8.39e8 floats
    x = np.concatenate([u.view(np.float32), np.array([0.0, 2.0 ** -60, np.nextafter(np.float32(2.0 ** 40), np.float32(0))], np.float32)])
    got = device_eval(tmp_path, 9, x)
    want = x / np.float32(299792458.0)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, "%d of %d differ, e.g. x=0x%08x got 0x%08x want 0x%08x" % (
        bad.size, x.size, bits(x)[bad[0]], bits(got)[bad[0]], bits(want)[bad[0]])


# s and s1_alpha of the 17 materials (csrc/host/materials.c)
MATERIALS = [(0.1, 2), (0.5, 4), (0.4, 3), (0.3, 3), (0.2, 2), (0.3, 3), (0.3, 3), (0.2, 2), (0.2, 2), (0.4, 3), (0.3, 3),
             (0.3, 3), (0.3, 3), (0.0, 1), (0.4, 4), (0.5, 4), (0.5, 4)]


def scatter_grid():
    """(s, alpha, theta_s, theta_i) of the grid: theta_s over [0, pi] (the acos of any cosine), theta_i over
    [0, pi/2] (a folded incidence angle), both with their end points and values next to them."""
    th_s = np.linspace(0.0, np.pi, 16).astype(np.float32)
    th_i = np.linspace(0.0, np.pi / 2, 16).astype(np.float32)
    th_s[1], th_i[1] = np.float32(1e-7), np.float32(3e-4)
    m, a, b = np.meshgrid(np.arange(len(MATERIALS)), th_s, th_i, indexing="ij")
    sa = np.array(MATERIALS, np.float32)[m.reshape(-1)]
    return np.stack([sa[:, 0], sa[:, 1], a.reshape(-1), b.reshape(-1)], axis=1).astype(np.float32)


def test_scatter_pattern_grid(tmp_path):
    x = scatter_grid()
    got = device_eval(tmp_path, 10, x.reshape(-1)).reshape(-1, 4)
    want = np.load(GOLDEN)
    assert want.shape == got.shape and want.dtype == np.float32
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, "%d values differ, e.g. item %d (s, alpha, th_s, th_i) = %s: got %s want %s" % (
        len(bad), bad[0][0], x[bad[0][0]], got[bad[0][0]], want[bad[0][0]])
    nrm = np.sqrt((want.astype(np.float64) ** 2).sum(axis=1))
    assert (np.abs(nrm - 1.0) < 1e-6).sum() > 0.9 * len(nrm)   # normalised wherever the pattern is not zero
