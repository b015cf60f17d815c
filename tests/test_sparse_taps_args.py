"""Argument checks of the sparse taps entries (hrt_sparse_array_taps, hrt_compute_sparse_array_taps,
hermespy_rt.compute_sparse_array_taps, Tracer.sparse_array_taps): a refused call returns HRT_E_INVALID before the device
is touched, so these run without a GPU.  hrt_sparse_array_taps has no problem handle that a test could leave out, so a
spec is shown to pass a check by the LAST check of the entry then refusing the call (accumulate = 2), never by a launch
on made-up pointers.  Without a device a valid call fails loudly (HRT_E_HIP), never with a CPU result."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi

from . import configs as K
from . import sparse_taps_util as U

HRT_E_INVALID, HRT_E_HIP = -1, -3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000   # a stand-in for a device pointer: tested for NULL and alignment only, never read
FIELDS = ["fs_hz", "fc_hz", "t0_s", "dt_s", "l_min", "num_taps", "num_times", "num_rx", "num_tx", "max_paths"]
WHO = b"hrt_sparse_array_taps"


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _el(n):
    return np.arange(3 * n, dtype=np.float32).reshape(n, 3) * 1e-3


def _spec(**over):
    kw = dict(num_rx=2, num_tx=3, max_paths=8, fs=30.72e6, num_taps=5, l_min=-2, fc=3.5e9, t0=0.0, dt=1e-3, num_times=2)
    kw.update(over)
    return abi.sparse_taps_spec(**kw)


def test_sparse_taps_spec_struct_matches_c(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hermespy_rt.h"\n'
                    'int main(void){printf("%zu' + ' %zu' * len(FIELDS) + '\\n", sizeof(hrt_sparse_taps_spec)' +
                    "".join(", offsetof(hrt_sparse_taps_spec, %s)" % f for f in FIELDS) + ');return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = abi.SparseTapsSpec
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in FIELDS]


# name -> (spec overrides, what the message names)
BAD_SPEC = {
    "zero_num_rx": (dict(num_rx=0), "num_rx * num_tx = 0"),
    "zero_num_tx": (dict(num_tx=0), "num_rx * num_tx = 0"),
    "links_65536": (dict(num_rx=256, num_tx=256, max_paths=1), "num_rx * num_tx = 65536"),
    "links_wrap_32_bits": (dict(num_rx=1 << 16, num_tx=1 << 16, max_paths=1), "num_rx * num_tx = 4294967296"),
    "zero_max_paths": (dict(max_paths=0), "max_paths = 0"),
    "max_paths_1025": (dict(max_paths=1025), "max_paths = 1025"),
    "link_paths_over_2_22": (dict(num_rx=64, num_tx=65, max_paths=1024), "2^22"),
    "zero_num_taps": (dict(num_taps=0), "num_taps"),
    "zero_num_times": (dict(num_times=0), "num_times"),
    "grid_over_2_20": (dict(num_taps=1 << 10, num_times=(1 << 10) + 1), "2^20"),
    "fs_nan": (dict(fs=math.nan), "sampling rate"),
    "fs_inf": (dict(fs=math.inf), "sampling rate"),
    "fs_zero": (dict(fs=0.0), "sampling rate"),
    "fs_negative": (dict(fs=-1e6), "sampling rate"),
    "fc_nan": (dict(fc=math.nan), "finite"),
    "t0_inf": (dict(t0=-math.inf), "finite"),
    "dt_nan": (dict(dt=math.nan), "finite"),
    "l_min_below": (dict(l_min=-(1 << 24) - 1), "2^24"),
    "l_min_above": (dict(l_min=(1 << 24) + 1, num_taps=1), "2^24"),
    "last_tap_above": (dict(l_min=(1 << 24) - 4, num_taps=5), "2^24"),
}

# name -> (keyword arguments of _device_call, what the message names)
BAD_ARRAYS = {
    "zero_nr": (dict(nr=0), "0 RX and 2 TX elements"),
    "zero_nt": (dict(nt=0), "4 RX and 0 TX elements"),
    "nr_1025": (dict(nr=1025), "1025 RX"),
    "nt_1025": (dict(nt=1025), "1025 TX"),
    "points_over_2_24": (dict(nr=64, nt=16, spec=dict(num_taps=129, num_times=128)), "2^24"),
    "fa_nan": (dict(fa=math.nan), "array frequency"),
    "fa_inf": (dict(fa=math.inf), "array frequency"),
    "fa_zero": (dict(fa=0.0), "array frequency"),
    "fa_negative": (dict(fa=-3.5e9), "array frequency"),
    "null_rx_elements": (dict(rx_el=None), "NULL element offsets"),
    "null_tx_elements": (dict(tx_el=None), "NULL element offsets"),
    "null_paths": (dict(paths=None), "NULL device pointer"),
    "null_out": (dict(out=None), "NULL device pointer"),
    "paths_not_aligned": (dict(paths=PTR + 4), "8-byte aligned"),
    "accumulate_2": (dict(accumulate=2), "accumulate must be 0 or 1"),
    "accumulate_negative": (dict(accumulate=-1), "accumulate must be 0 or 1"),
}

# the largest values that pass every check before the last
AT_LIMIT = {
    "links_65535": dict(spec=dict(num_rx=255, num_tx=257, max_paths=64)),
    "max_paths_1024": dict(spec=dict(max_paths=1024)),
    "link_paths_2_22": dict(spec=dict(num_rx=64, num_tx=64, max_paths=1024)),
    "grid_2_20": dict(nr=4, nt=4, spec=dict(num_taps=1 << 10, num_times=1 << 10)),
    "elements_1024": dict(nr=1024, nt=1024, spec=dict(num_taps=4, num_times=4)),
    "points_2_24": dict(nr=64, nt=16, spec=dict(num_taps=128, num_times=128)),
    "l_min_lowest": dict(spec=dict(l_min=-(1 << 24))),
    "last_tap_highest": dict(spec=dict(l_min=(1 << 24) - 5, num_taps=5)),
    "fc_zero_dt_zero": dict(spec=dict(fc=0.0, dt=0.0)),
    "all_ones": dict(nr=1, nt=1, spec=dict(num_rx=1, num_tx=1, max_paths=1, num_taps=1, num_times=1)),
}


def test_size_function(product_lib):
    L = product_lib
    for nrx, ntx, k, nl, nt, nr, nte in ((1, 1, 1, 1, 1, 1, 1), (2, 3, 8, 5, 2, 4, 6), (255, 257, 64, 16, 1, 2, 2),
                                         (64, 64, 1024, 1 << 10, 1 << 10, 1, 1)):
        spec = _spec(num_rx=nrx, num_tx=ntx, max_paths=k, num_taps=nl, num_times=nt)
        want = nrx * ntx * nr * nte * 2 * nt * nl * 8
        assert L.hrt_sparse_taps_out_bytes(C.byref(spec), nr, nte) == want == abi.sparse_taps_out_bytes(spec, nr, nte)
    assert L.hrt_sparse_taps_out_bytes(None, 1, 1) == 0
    for bad in sorted(BAD_SPEC):
        spec = _spec(**BAD_SPEC[bad][0])
        assert L.hrt_sparse_taps_out_bytes(C.byref(spec), 2, 2) == 0 == abi.sparse_taps_out_bytes(spec, 2, 2), bad
    for name in sorted(AT_LIMIT):
        spec = _spec(**AT_LIMIT[name].get("spec", {}))
        assert L.hrt_sparse_taps_out_bytes(C.byref(spec), 1, 1) == abi.sparse_taps_out_bytes(spec, 1, 1) > 0, name


def _device_call(lib, spec=None, rx_el=PTR, nr=4, tx_el=PTR, nt=2, fa=3.5e9, paths=PTR, out=PTR, accumulate=0):
    sp = _spec(**(spec or {}))
    rc = lib.hrt_sparse_array_taps(0, C.byref(sp), rx_el, nr, tx_el, nt, C.c_double(fa), paths, out, accumulate, None)
    return rc, lib.hrt_last_error()


@pytest.mark.parametrize("bad", sorted(BAD_SPEC))
def test_device_entry_refuses_the_spec(product_lib, bad):
    over, what = BAD_SPEC[bad]
    rc, msg = _device_call(product_lib, spec=over)
    assert rc == HRT_E_INVALID and WHO in msg and what.encode() in msg, msg


@pytest.mark.parametrize("bad", sorted(BAD_ARRAYS))
def test_device_entry_refuses_the_arrays_and_pointers(product_lib, bad):
    kw, what = BAD_ARRAYS[bad]
    rc, msg = _device_call(product_lib, **kw)
    assert rc == HRT_E_INVALID and WHO in msg and what.encode() in msg, msg


@pytest.mark.parametrize("name", sorted(AT_LIMIT))
def test_device_entry_accepts_the_call_at_its_limits(product_lib, name):
    rc, msg = _device_call(product_lib, accumulate=2, **AT_LIMIT[name])
    assert rc == HRT_E_INVALID and b"accumulate must be 0 or 1" in msg, msg


def test_device_entry_refuses_a_null_spec(product_lib):
    L = product_lib
    assert L.hrt_sparse_array_taps(0, None, PTR, 1, PTR, 1, C.c_double(1e9), PTR, PTR, 0, None) == HRT_E_INVALID
    assert b"hrt_sparse_array_taps: NULL spec" in L.hrt_last_error()
    with pytest.raises(RuntimeError, match=r"hrt_sparse_array_taps failed \(-1\)"):
        abi.run_sparse_array_taps(L, 0, _spec(), PTR, 4, PTR, 2, 3.5e9, None, PTR)


# ---------------------------------------------------------------------------------------------- the drop-in entry

def _drop_in(lib, nr=4, nt=2, num_times=1, num_taps=4, l_min=0, max_paths=8, parts=None, fa=3.5e9, fs=30.72e6,
             fc=3.5e9, out="array", rx_el=None, nrx=None, ntx=None, grid="spec", dominant="spec", paths=False):
    """hrt_compute_sparse_array_taps as called: every argument explicit, nothing derived (a refusal comes before any
    pointer is read, so the counts need not match the arrays) -> (rc, message)"""
    c = K.small(K.C1, 64)
    scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces = K.args(c)
    rx_pos = np.asarray(rx_pos, np.float32).reshape(-1, 3)
    tx_pos = np.asarray(tx_pos, np.float32).reshape(-1, 3)
    rx_vel = np.asarray(rx_vel, np.float32).reshape(-1, 3)
    tx_vel = np.asarray(tx_vel, np.float32).reshape(-1, 3)
    V3 = C.POINTER(abi.Vec3)
    gs = abi.taps_spec(fs, num_taps, l_min, fc, 0.0, 0.0, num_times, parts=0x55)   # (the grid's parts are not read)
    ds = abi.dominant_spec(max_paths, parts=abi.CHANNEL_LOS | abi.CHANNEL_SCATTER if parts is None else parts)
    re = _el(min(nr, 1025)) if rx_el is None else rx_el
    te = _el(min(nt, 1025))
    oa = np.zeros(1 << 12, np.float32)
    pa = np.zeros(1 << 12, np.uint8)
    scene = lib.scene_load(str(scene_path).encode())
    try:
        rc = lib.hrt_compute_sparse_array_taps(
            C.byref(scene), rx_pos.ctypes.data_as(V3), tx_pos.ctypes.data_as(V3), rx_vel.ctypes.data_as(V3),
            tx_vel.ctypes.data_as(V3), C.c_float(f_ghz), rx_pos.shape[0] if nrx is None else nrx,
            tx_pos.shape[0] if ntx is None else ntx, int(num_paths), int(num_bounces),
            C.byref(ds) if dominant == "spec" else None, C.byref(gs) if grid == "spec" else None,
            re.ctypes.data_as(V3), nr, te.ctypes.data_as(V3), nt, C.c_double(fa),
            oa.ctypes.data_as(C.POINTER(C.c_float)) if out == "array" else None,
            pa.ctypes.data_as(C.c_void_p) if paths else None, None)
    finally:
        abi.free_scene(scene)
    return rc, lib.hrt_last_error()


_NAN_EL = _el(4)
_NAN_EL[1, 2] = math.nan

# name -> (arguments of _drop_in, what the message names)
BAD_DROP_IN = {
    # hrt_compute_dominant_paths' refusals
    "null_dominant_spec": (dict(dominant=None), "NULL spec"),
    "zero_max_paths": (dict(max_paths=0), "max_paths = 0"),
    "max_paths_1025": (dict(max_paths=1025), "max_paths = 1025"),
    "no_parts": (dict(parts=0), "parts"),
    "unknown_part": (dict(parts=abi.CHANNEL_LOS | 4), "parts"),
    "links_65536": (dict(nrx=256, ntx=256, max_paths=1), "num_rx * num_tx = 65536"),
    "link_paths_over_2_22": (dict(nrx=64, ntx=65, max_paths=1024), "2^22"),
    "zero_num_rx": (dict(nrx=0), "must be > 0"),
    "zero_num_tx": (dict(ntx=0), "must be > 0"),
    # the grid's
    "null_grid": (dict(grid=None), "NULL grid"),
    "zero_num_taps": (dict(num_taps=0), "num_taps"),
    "zero_num_times": (dict(num_times=0), "num_times"),
    "grid_over_2_20": (dict(nr=1, nt=1, num_taps=1 << 10, num_times=(1 << 10) + 1), "2^20"),
    "fs_zero": (dict(fs=0.0), "sampling rate"),
    "fs_nan": (dict(fs=math.nan), "sampling rate"),
    "fc_inf": (dict(fc=math.inf), "finite"),
    "l_min_below": (dict(l_min=-(1 << 24) - 1), "2^24"),
    "last_tap_above": (dict(l_min=(1 << 24) - 3, num_taps=4), "2^24"),
    # the arrays'
    "zero_nr": (dict(nr=0), "0 RX and 2 TX elements"),
    "zero_nt": (dict(nt=0), "4 RX and 0 TX elements"),
    "nr_1025": (dict(nr=1025), "1025 RX"),
    "nt_1025": (dict(nt=1025), "1025 TX"),
    "points_over_2_24": (dict(nr=64, nt=16, num_times=128, num_taps=129), "2^24"),
    "fa_zero": (dict(fa=0.0), "array frequency"),
    "fa_negative": (dict(fa=-1.0), "array frequency"),
    "fa_inf": (dict(fa=math.inf), "array frequency"),
    "fa_nan": (dict(fa=math.nan), "array frequency"),
    "offset_not_finite": (dict(rx_el=_NAN_EL), "RX element 1"),
    "null_out": (dict(out=None), "hrt_compute_sparse_array_taps: NULL argument"),
    "null_out_with_paths": (dict(out=None, paths=True), "hrt_compute_sparse_array_taps: NULL argument"),
}


@pytest.mark.parametrize("bad", sorted(BAD_DROP_IN))
def test_drop_in_refuses_invalid_call(product_lib, bad):
    kw, what = BAD_DROP_IN[bad]
    rc, msg = _drop_in(product_lib, **kw)
    assert rc == HRT_E_INVALID, msg
    assert what.encode() in msg, msg


def test_runner_reports_a_refusal(product_lib):
    c = K.small(K.C1, 64)
    grid = abi.taps_spec(30.72e6, 4)
    with pytest.raises(RuntimeError, match=r"hrt_compute_sparse_array_taps failed \(-1\)"):
        abi.run_compute_sparse_array_taps(product_lib, *K.args(c), abi.dominant_spec(1025), grid, _el(4), _el(2))
    assert b"max_paths = 1025" in product_lib.hrt_last_error()
    with pytest.raises(RuntimeError, match=r"hrt_compute_sparse_array_taps failed \(-1\)"):
        abi.run_compute_sparse_array_taps(product_lib, *K.args(c), abi.dominant_spec(8), grid, _el(1025), _el(2),
                                          return_paths=True)
    assert b"1025 RX" in product_lib.hrt_last_error()


# ---------------------------------------------------------------------------------------------- the pybind entry

def _pybind():
    import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    return hermespy_rt


PYBIND_BAD = {
    "zero_max_paths": (dict(max_paths=0), "max_paths = 0"),
    "max_paths_1025": (dict(max_paths=1025), "max_paths = 1025"),
    "no_parts": (dict(los=False, scatter=False), "parts"),
    "zero_nr": (dict(rx_elements=np.zeros((0, 3), np.float32)), "0 RX and 2 TX elements"),
    "nt_1025": (dict(tx_elements=_el(1025)), "1025 TX"),
    "zero_num_taps": (dict(num_taps=0), "num_taps"),
    "zero_num_times": (dict(num_times=0), "num_times"),
    "grid_over_2_20": (dict(rx_elements=_el(1), tx_elements=_el(1), num_times=1 << 10, num_taps=(1 << 10) + 1), r"2\^20"),
    "points_over_2_24": (dict(rx_elements=_el(64), tx_elements=_el(16), num_times=128, num_taps=129), r"2\^24"),
    "fa_nan": (dict(array_frequency=math.nan), "array frequency"),
    "fa_zero": (dict(array_frequency=0.0), "array frequency"),
    "fs_zero": (dict(sampling_rate=0.0), "sampling rate"),
    "fc_inf": (dict(center_frequency=math.inf), "finite"),
    "l_min_below": (dict(l_min=-(1 << 24) - 1), r"2\^24"),
    "l_min_far_below": (dict(l_min=-(1 << 31)), r"2\^24"),
    "offset_not_finite": (dict(rx_elements=_NAN_EL), "RX element 1"),
    "return_paths_refused_alike": (dict(max_paths=1025, return_paths=True), "max_paths = 1025"),
}


@pytest.mark.parametrize("bad", sorted(PYBIND_BAD))
def test_pybind_refuses_invalid_call(bad):
    hermespy_rt = _pybind()
    c = K.small(K.C1, 64)
    args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], 1, 1, 64, 1)
    kw = dict(sampling_rate=30.72e6, num_taps=4, rx_elements=_el(4), tx_elements=_el(2), max_paths=8)
    over, what = PYBIND_BAD[bad]
    kw.update(over)
    with pytest.raises(ValueError, match=what):
        hermespy_rt.compute_sparse_array_taps(*args, **kw)


def test_pybind_refuses_too_many_links():
    hermespy_rt = _pybind()
    c = K.small(K.C1, 64)
    pos = np.zeros((256, 3), np.float32)
    with pytest.raises(ValueError, match="num_rx \\* num_tx = 65536"):
        hermespy_rt.compute_sparse_array_taps(c["scene_path"], pos, pos, pos, pos, c["f_ghz"], 256, 256, 64, 1,
                                              sampling_rate=30.72e6, num_taps=4, rx_elements=_el(1),
                                              tx_elements=_el(1), max_paths=1)


# ---------------------------------------------------------------------------------------------- Tracer's own checks

def _bare_tracer(nrx=2, ntx=3):
    """a Tracer without a problem or a device behind it: the list checks of sparse_array_taps come before anything
    touches the device, so they run on it (a GPU test runs the same calls on a real one)"""
    import torch
    from hermespy_rt_amd.device import Tracer
    tr = Tracer.__new__(Tracer)
    tr.torch, tr.device, tr.nrx, tr.ntx, tr.f_ghz = torch, torch.device("cuda", 0), nrx, ntx, 3.5
    tr.close = lambda: None
    return tr


def test_tracer_refuses_lists_of_the_wrong_dtype_device_or_size():
    U.tracer_value_errors(_bare_tracer())


def test_sparse_taps_without_device_fails_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny call
    succeeds and returns finite taps and the lists.)"""
    c = K.small(K.C1, 64)
    call = lambda: abi.run_compute_sparse_array_taps(product_lib, *K.args(c), abi.dominant_spec(8),   # noqa: E731
                                                     abi.taps_spec(30.72e6, 64, fc=3.5e9), _el(4), _el(2),
                                                     return_paths=True)
    if _have_gpu():
        h, v = call()
        assert h.shape == (1, 1, 4, 2, 2, 1, 64) and np.isfinite(h).all() and np.abs(h).max() > 0
        assert v["kept"].shape == (1, 1) and int(v["kept"][0, 0]) == 8 and int(v["eligible"][0, 0]) > 8
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_sparse_array_taps failed \(-3\)") as e:
        call()
    assert "HIP" in str(e.value)
