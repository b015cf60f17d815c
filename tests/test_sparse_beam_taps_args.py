"""Argument checks of the sparse beam taps entries (hrt_sparse_beam_taps, hrt_compute_sparse_beam_taps,
hermespy_rt.compute_sparse_beam_taps, Tracer.sparse_beam_taps): a refused call returns HRT_E_INVALID before the device
is touched, so these run without a GPU.  hrt_sparse_beam_taps has no problem handle that a test could leave out, so a call is shown to pass a check by the LAST check of the entry then refusing it (accumulate = 2), never by a
launch on made-up pointers.  Without a device a valid call fails loudly (HRT_E_HIP), never with a CPU result."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi, lib

from . import configs as K
from . import sparse_beam_taps_util as U
from .test_sparse_taps_args import BAD_SPEC, _spec

HRT_E_INVALID, HRT_E_HIP = -1, -3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000   # a stand-in for a device pointer: tested for NULL and alignment only, never read
WHO = b"hrt_sparse_beam_taps"


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _el(n):
    return np.arange(3 * n, dtype=np.float32).reshape(n, 3) * 1e-3


def _w(b, n):
    return (np.arange(b * n).reshape(b, n) % 5 - 2 + 1j * (np.arange(b * n).reshape(b, n) % 3 + 1)).astype(np.complex64)


def test_size_function(product_lib):
    L = product_lib
    for nrx, ntx, k, nk, nt, br, bt in ((1, 1, 1, 1, 1, 1, 1), (2, 3, 8, 5, 2, 4, 6), (255, 257, 64, 16, 1, 2, 2),
                                        (64, 64, 1024, 1 << 10, 1 << 10, 1, 1)):
        spec = _spec(num_rx=nrx, num_tx=ntx, max_paths=k, num_taps=nk, num_times=nt)
        want = nrx * ntx * br * bt * 2 * nt * nk * 8
        assert L.hrt_sparse_beam_taps_out_bytes(C.byref(spec), br, bt) == want == abi.sparse_beam_taps_out_bytes(spec, br, bt)
    assert L.hrt_sparse_beam_taps_out_bytes(None, 1, 1) == 0
    for bad in sorted(BAD_SPEC):
        spec = _spec(**BAD_SPEC[bad][0])
        assert L.hrt_sparse_beam_taps_out_bytes(C.byref(spec), 2, 2) == 0 == abi.sparse_beam_taps_out_bytes(spec, 2, 2), bad


# name -> (keyword arguments of _device_call, what the message names)
BAD_CALL = {
    "zero_nr": (dict(nr=0), "0 RX and 2 TX elements"),
    "zero_nt": (dict(nt=0), "4 RX and 0 TX elements"),
    "nr_257": (dict(nr=257), "257 RX and 2 TX elements"),
    "nt_257": (dict(nt=257), "4 RX and 257 TX elements"),
    "zero_br": (dict(br=0), "0 RX and 5 TX beams"),
    "zero_bt": (dict(bt=0), "3 RX and 0 TX beams"),
    "br_257": (dict(br=257), "257 RX and 5 TX beams"),
    "bt_257": (dict(bt=257), "3 RX and 257 TX beams"),
    "points_over_2_24": (dict(br=64, bt=16, spec=dict(num_taps=129, num_times=128)), "2^24"),
    "fa_nan": (dict(fa=math.nan), "array frequency"),
    "fa_inf": (dict(fa=math.inf), "array frequency"),
    "fa_zero": (dict(fa=0.0), "array frequency"),
    "fa_negative": (dict(fa=-3.5e9), "array frequency"),
    "null_rx_elements": (dict(rx_el=None), "NULL device pointer"),
    "null_tx_elements": (dict(tx_el=None), "NULL device pointer"),
    "null_rx_weights": (dict(rx_w=None), "NULL device pointer"),
    "null_tx_weights": (dict(tx_w=None), "NULL device pointer"),
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
    "grid_2_20": dict(br=4, bt=4, spec=dict(num_taps=1 << 10, num_times=1 << 10)),
    "elements_and_beams_256": dict(nr=256, nt=256, br=256, bt=256, spec=dict(num_taps=16, num_times=16)),
    "points_2_24": dict(br=64, bt=16, spec=dict(num_taps=128, num_times=128)),
    # 256 x 256 elements at 512 taps: 2^25 points of the element-domain taps, which are never formed
    "elements_beyond_the_array_taps": dict(nr=256, nt=256, br=4, bt=4, spec=dict(num_taps=512, num_times=1)),
    "taps_up_to_2_24": dict(spec=dict(l_min=(1 << 24) - 5, num_taps=5)),
    "taps_from_minus_2_24": dict(spec=dict(l_min=-(1 << 24))),
    "all_ones": dict(nr=1, nt=1, br=1, bt=1, spec=dict(num_rx=1, num_tx=1, max_paths=1, num_taps=1, num_times=1)),
}


def _device_call(L, spec=None, rx_el=PTR, nr=4, tx_el=PTR, nt=2, fa=3.5e9, rx_w=PTR, br=3, tx_w=PTR, bt=5, paths=PTR,
                 out=PTR, accumulate=0):
    sp = _spec(**(spec or {}))
    rc = L.hrt_sparse_beam_taps(0, C.byref(sp), rx_el, nr, tx_el, nt, C.c_double(fa), rx_w, br, tx_w, bt, paths, out,
                                   accumulate, None)
    return rc, L.hrt_last_error()


@pytest.mark.parametrize("bad", sorted(BAD_SPEC))
def test_device_entry_refuses_every_sparse_spec_refusal(product_lib, bad):
    over, what = BAD_SPEC[bad]
    rc, msg = _device_call(product_lib, spec=over)
    assert rc == HRT_E_INVALID and what.encode() in msg, msg
    assert WHO in msg, msg


@pytest.mark.parametrize("bad", sorted(BAD_CALL))
def test_device_entry_refuses_the_counts_and_pointers(product_lib, bad):
    kw, what = BAD_CALL[bad]
    rc, msg = _device_call(product_lib, **kw)
    assert rc == HRT_E_INVALID and WHO in msg and what.encode() in msg, msg


@pytest.mark.parametrize("name", sorted(AT_LIMIT))
def test_device_entry_accepts_the_call_at_its_limits(product_lib, name):
    rc, msg = _device_call(product_lib, accumulate=2, **AT_LIMIT[name])
    assert rc == HRT_E_INVALID and b"accumulate must be 0 or 1" in msg, msg


def test_the_array_taps_of_a_list_refuse_what_the_beam_taps_accept(product_lib):
    L = product_lib
    sp = _spec(num_taps=512, num_times=1)
    rc = L.hrt_sparse_array_taps(0, C.byref(sp), PTR, 256, PTR, 256, C.c_double(3.5e9), PTR, PTR, 2, None)
    assert rc == HRT_E_INVALID and b"2^24" in L.hrt_last_error()


def test_device_entry_refuses_a_null_spec(product_lib):
    L = product_lib
    assert L.hrt_sparse_beam_taps(0, None, PTR, 1, PTR, 1, C.c_double(1e9), PTR, 1, PTR, 1, PTR, PTR, 0,
                                     None) == HRT_E_INVALID
    assert b"hrt_sparse_beam_taps: NULL spec" in L.hrt_last_error()
    with pytest.raises(RuntimeError, match=r"hrt_sparse_beam_taps failed \(-1\)"):
        abi.run_sparse_beam_taps(L, 0, _spec(), PTR, 4, PTR, 2, 3.5e9, PTR, 3, PTR, 5, None, PTR)


# ---------------------------------------------------------------------------------------------- the drop-in entry

def _drop_in(L, nr=4, nt=2, br=3, bt=5, num_times=1, num_taps=4, l_min=0, max_paths=8, parts=None, fa=3.5e9, fs=30.72e6,
             fc=3.5e9, out="array",
             rx_el=None, rx_w="array", tx_w="array", nrx=None, ntx=None, grid="spec", dominant="spec", paths=False):
    """hrt_compute_sparse_beam_taps as called: every argument explicit, nothing derived (a refusal of a count comes
    before any pointer is read, so the counts need not match the arrays) -> (rc, message)"""
    c = K.small(K.C1, 64)
    scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces = K.args(c)
    rx_pos = np.asarray(rx_pos, np.float32).reshape(-1, 3)
    tx_pos = np.asarray(tx_pos, np.float32).reshape(-1, 3)
    rx_vel = np.asarray(rx_vel, np.float32).reshape(-1, 3)
    tx_vel = np.asarray(tx_vel, np.float32).reshape(-1, 3)
    V3, FP = C.POINTER(abi.Vec3), C.POINTER(C.c_float)
    gs = abi.taps_spec(fs, num_taps, l_min, fc, 0.0, 0.0, num_times, parts=0x55)   # (the grid's parts are not read)
    ds = abi.dominant_spec(max_paths, parts=abi.CHANNEL_LOS | abi.CHANNEL_SCATTER if parts is None else parts)
    re = _el(min(nr, 257)) if rx_el is None else rx_el
    te = _el(min(nt, 257))
    wr = _w(min(br, 257), min(nr, 257)) if isinstance(rx_w, str) else rx_w
    wt = _w(min(bt, 257), min(nt, 257)) if isinstance(tx_w, str) else tx_w
    oa = np.zeros(1 << 12, np.float32)
    pa = np.zeros(1 << 12, np.uint8)
    scene = L.scene_load(str(scene_path).encode())
    try:
        rc = L.hrt_compute_sparse_beam_taps(
            C.byref(scene), rx_pos.ctypes.data_as(V3), tx_pos.ctypes.data_as(V3), rx_vel.ctypes.data_as(V3),
            tx_vel.ctypes.data_as(V3), C.c_float(f_ghz), rx_pos.shape[0] if nrx is None else nrx,
            tx_pos.shape[0] if ntx is None else ntx, int(num_paths), int(num_bounces),
            C.byref(ds) if dominant == "spec" else None, C.byref(gs) if grid == "spec" else None,
            re.ctypes.data_as(V3), nr, te.ctypes.data_as(V3), nt, C.c_double(fa),
            wr.ctypes.data_as(FP) if wr is not None else None, br, wt.ctypes.data_as(FP) if wt is not None else None, bt,
            oa.ctypes.data_as(FP) if out == "array" else None, pa.ctypes.data_as(C.c_void_p) if paths else None, None)
    finally:
        abi.free_scene(scene)
    return rc, L.hrt_last_error()


_NAN_EL = _el(4)
_NAN_EL[1, 2] = math.nan
_INF_W = _w(5, 2)
_INF_W[4, 1] = complex(1.0, math.inf)

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
    "grid_over_2_20": (dict(br=1, bt=1, num_taps=1 << 10, num_times=(1 << 10) + 1), "2^20"),
    "fs_zero": (dict(fs=0.0), "sampling rate"),
    "fs_nan": (dict(fs=math.nan), "sampling rate"),
    "fc_inf": (dict(fc=math.inf), "finite"),
    "l_min_below": (dict(l_min=-(1 << 24) - 1), "2^24"),
    "last_tap_above": (dict(l_min=(1 << 24) - 3, num_taps=4), "2^24"),
    # the arrays' and the codebooks'
    "zero_nr": (dict(nr=0), "0 RX and 2 TX elements"),
    "zero_nt": (dict(nt=0), "4 RX and 0 TX elements"),
    "nr_257": (dict(nr=257), "257 RX"),
    "nt_257": (dict(nt=257), "257 TX"),
    "zero_br": (dict(br=0), "0 RX and 5 TX beams"),
    "zero_bt": (dict(bt=0), "3 RX and 0 TX beams"),
    "br_257": (dict(br=257), "257 RX and 5 TX beams"),
    "bt_257": (dict(bt=257), "3 RX and 257 TX beams"),
    "points_over_2_24": (dict(br=64, bt=16, num_times=128, num_taps=129), "2^24"),
    "fa_zero": (dict(fa=0.0), "array frequency"),
    "fa_negative": (dict(fa=-1.0), "array frequency"),
    "fa_inf": (dict(fa=math.inf), "array frequency"),
    "fa_nan": (dict(fa=math.nan), "array frequency"),
    "offset_not_finite": (dict(rx_el=_NAN_EL), "RX element 1"),
    "weight_not_finite": (dict(tx_w=_INF_W), "TX weight (4, 1)"),
    "null_rx_weights": (dict(rx_w=None), "NULL beam weights"),
    "null_tx_weights": (dict(tx_w=None), "NULL beam weights"),
    "null_out": (dict(out=None), "hrt_compute_sparse_beam_taps: NULL argument"),
    "null_out_with_paths": (dict(out=None, paths=True), "hrt_compute_sparse_beam_taps: NULL argument"),
}


@pytest.mark.parametrize("bad", sorted(BAD_DROP_IN))
def test_drop_in_refuses_invalid_call(product_lib, bad):
    kw, what = BAD_DROP_IN[bad]
    rc, msg = _drop_in(product_lib, **kw)
    assert rc == HRT_E_INVALID, msg
    assert what.encode() in msg, msg


def test_runner_reports_a_refusal(product_lib):
    c = K.small(K.C1, 64)
    grid = abi.taps_spec(30.72e6, 4, 0, 3.5e9)
    with pytest.raises(RuntimeError, match=r"hrt_compute_sparse_beam_taps failed \(-1\)"):
        abi.run_compute_sparse_beam_taps(product_lib, *K.args(c), abi.dominant_spec(1025), grid, _el(4), _el(2),
                                            _w(3, 4), _w(5, 2))
    assert b"max_paths = 1025" in product_lib.hrt_last_error()
    with pytest.raises(RuntimeError, match=r"hrt_compute_sparse_beam_taps failed \(-1\)"):
        abi.run_compute_sparse_beam_taps(product_lib, *K.args(c), abi.dominant_spec(8), grid, _el(4), _el(2),
                                            _w(257, 4), _w(5, 2), return_paths=True)
    assert b"257 RX and 5 TX beams" in product_lib.hrt_last_error()
    with pytest.raises(ValueError, match=r"tx_weights must have shape \(beams, 2\)"):
        abi.run_compute_sparse_beam_taps(product_lib, *K.args(c), abi.dominant_spec(8), grid, _el(4), _el(2),
                                            _w(3, 4), _w(5, 3))


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
    "zero_nr": (dict(rx_elements=np.zeros((0, 3), np.float32), rx_weights=np.zeros((3, 0), np.complex64)),
                "0 RX and 2 TX elements"),
    "nt_257": (dict(tx_elements=_el(257), tx_weights=_w(5, 257)), "257 TX"),
    "zero_br": (dict(rx_weights=np.zeros((0, 4), np.complex64)), "0 RX and 5 TX beams"),
    "bt_257": (dict(tx_weights=_w(257, 2)), "3 RX and 257 TX beams"),
    "zero_num_taps": (dict(num_taps=0), "num_taps"),
    "zero_num_times": (dict(num_times=0), "num_times"),
    "grid_over_2_20": (dict(num_times=1 << 10, num_taps=(1 << 10) + 1), r"2\^20"),
    "points_over_2_24": (dict(rx_weights=_w(64, 4), tx_weights=_w(16, 2), num_times=128, num_taps=129), r"2\^24"),
    "fa_nan": (dict(array_frequency=math.nan), "array frequency"),
    "fa_zero": (dict(array_frequency=0.0), "array frequency"),
    "fs_zero": (dict(sampling_rate=0.0), "sampling rate"),
    "fc_inf": (dict(center_frequency=math.inf), "finite"),
    "l_min_below": (dict(l_min=-(1 << 24) - 1), r"2\^24"),
    "l_min_far_below": (dict(l_min=-(1 << 31)), r"2\^24"),
    "offset_not_finite": (dict(rx_elements=_NAN_EL), "RX element 1"),
    "weight_not_finite": (dict(tx_weights=_INF_W), r"TX weight \(4, 1\)"),
    "return_paths_refused_alike": (dict(max_paths=1025, return_paths=True), "max_paths = 1025"),
}


@pytest.mark.parametrize("bad", sorted(PYBIND_BAD))
def test_pybind_refuses_invalid_call(bad):
    hermespy_rt = _pybind()
    c = K.small(K.C1, 64)
    args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], 1, 1, 64, 1)
    kw = dict(sampling_rate=30.72e6, num_taps=4, rx_elements=_el(4), tx_elements=_el(2), rx_weights=_w(3, 4),
              tx_weights=_w(5, 2), max_paths=8)
    over, what = PYBIND_BAD[bad]
    kw.update(over)
    with pytest.raises(ValueError, match=what):
        hermespy_rt.compute_sparse_beam_taps(*args, **kw)


def test_pybind_refuses_too_many_links():
    hermespy_rt = _pybind()
    c = K.small(K.C1, 64)
    pos = np.zeros((256, 3), np.float32)
    with pytest.raises(ValueError, match="num_rx \\* num_tx = 65536"):
        hermespy_rt.compute_sparse_beam_taps(c["scene_path"], pos, pos, pos, pos, c["f_ghz"], 256, 256, 64, 1,
                                             sampling_rate=30.72e6, num_taps=4, rx_elements=_el(1), tx_elements=_el(1),
                                             rx_weights=_w(1, 1), tx_weights=_w(1, 1), max_paths=1)


# ---------------------------------------------------------------------------------------------- Tracer's own checks

def _bare_tracer(nrx=2, ntx=3):
    """a Tracer without a problem or a device behind it: the list, element and weight checks of sparse_beam_taps
    come before anything touches the device, so they run on it (a GPU test runs the same calls on a real one)"""
    import torch
    from hermespy_rt_amd.device import Tracer
    tr = Tracer.__new__(Tracer)
    tr.torch, tr.device, tr.nrx, tr.ntx, tr.f_ghz = torch, torch.device("cuda", 0), nrx, ntx, 3.5
    tr.close = lambda: None
    return tr


def test_tracer_refuses_lists_elements_and_weights_that_are_its_own_to_refuse():
    U.tracer_value_errors(_bare_tracer())


def test_export_list_covers_the_sparse_beam_taps_entries(product_lib):
    names = ("hrt_sparse_beam_taps_out_bytes", "hrt_sparse_beam_taps", "hrt_compute_sparse_beam_taps")
    for n in names:
        assert n in lib.EXPORTED
        assert getattr(product_lib, n).argtypes is not None, n
    exports = open(os.path.join(REPO, "hermespy-rt_amd", "csrc", "exports.map")).read()
    headers = "".join(open(os.path.join(REPO, "include", h)).read() for h in ("hermespy_rt.h", "hrt_device.h"))
    for n in names:
        assert n + ";" in exports and n + "(" in headers


def test_sparse_beam_taps_without_device_fails_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny call
    succeeds and returns finite beam taps and the lists.)"""
    c = K.small(K.C1, 64)
    call = lambda: abi.run_compute_sparse_beam_taps(product_lib, *K.args(c), abi.dominant_spec(8),   # noqa: E731
                                                       abi.taps_spec(30.72e6, 4, 0, 3.5e9), _el(4), _el(2), _w(3, 4),
                                                       _w(5, 2), return_paths=True)
    if _have_gpu():
        B, v = call()
        assert B.shape == (1, 1, 3, 5, 2, 1, 4) and np.isfinite(B).all() and np.abs(B).max() > 0
        assert v["kept"].shape == (1, 1) and int(v["kept"][0, 0]) == 8 and int(v["eligible"][0, 0]) > 8
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_sparse_beam_taps failed \(-3\)") as e:
        call()
    assert "HIP" in str(e.value)
