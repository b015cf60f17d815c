"""Argument checks of the antenna-array taps entries (hrt_array_taps_scratch_bytes, hrt_array_taps,
hrt_compute_array_taps, hermespy_rt.compute_array_taps): a refused call returns HRT_E_INVALID before the device is
touched, so these run without a GPU.  Every message names the new entry.  Without a device a valid call fails loudly
(HRT_E_HIP), never with a CPU result."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi, lib

from . import configs as K

HRT_E_INVALID, HRT_E_HIP = -1, -3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 122.88e6

ONE = [[0.0, 0.0, 0.0]]
ULA2 = [[0.0, 0.0, 0.0], [0.0, 0.05, 0.0]]

# name -> (spec overrides, rx_elements, tx_elements, array frequency, what the message names)
BAD_CALLS = {
    # the taps spec (every hrt_taps check)
    "no_taps": ({"num_taps": 0}, ONE, ONE, 3e9, "num_taps"),
    "no_times": ({"num_times": 0}, ONE, ONE, 3e9, "num_times"),
    "taps_times_over_2_20": ({"num_taps": 1 << 10, "num_times": (1 << 10) + 1}, ONE, ONE, 3e9, "2^20"),
    "fs_zero": ({"fs": 0.0}, ONE, ONE, 3e9, "sampling rate"),
    "fs_nan": ({"fs": math.nan}, ONE, ONE, 3e9, "sampling rate"),
    "fs_inf": ({"fs": math.inf}, ONE, ONE, 3e9, "sampling rate"),
    "fc_nan": ({"fc": math.nan}, ONE, ONE, 3e9, "finite"),
    "t0_inf": ({"t0": math.inf}, ONE, ONE, 3e9, "finite"),
    "dt_nan": ({"dt": math.nan}, ONE, ONE, 3e9, "finite"),
    "l_min_below": ({"l_min": -(1 << 24) - 1}, ONE, ONE, 3e9, "2^24"),
    "l_min_above": ({"l_min": (1 << 24) + 1}, ONE, ONE, 3e9, "2^24"),
    "last_tap_above": ({"l_min": (1 << 24) - 63, "num_taps": 64}, ONE, ONE, 3e9, "2^24"),
    "no_parts": ({"parts": 0}, ONE, ONE, 3e9, "parts"),
    "unknown_part": ({"parts": abi.CHANNEL_SCATTER | 8}, ONE, ONE, 3e9, "parts"),
    # the arrays
    "no_rx_elements": ({}, np.zeros((0, 3)), ONE, 3e9, "elements"),
    "no_tx_elements": ({}, ONE, np.zeros((0, 3)), 3e9, "elements"),
    "rx_1025": ({}, np.zeros((1025, 3)), ONE, 3e9, "elements"),
    "tx_1025": ({"num_taps": 1}, ONE, np.zeros((1025, 3)), 3e9, "elements"),
    "over_2_24": ({"num_taps": 1 << 10, "num_times": 1 << 10}, ULA2, np.zeros((9, 3)), 3e9, "2^24"),
    "fa_zero": ({}, ONE, ONE, 0.0, "array frequency"),
    "fa_negative": ({}, ONE, ONE, -3e9, "array frequency"),
    "fa_nan": ({}, ONE, ONE, math.nan, "array frequency"),
    "fa_inf": ({}, ONE, ONE, math.inf, "array frequency"),
}
# offsets are checked where they are host memory (the C drop-in, pybind, Tracer), not in the device entry
BAD_OFFSETS = {
    "rx_nan": ([[0.0, math.nan, 0.0]], ONE),
    "tx_inf": (ONE, [[0.0, 0.0, 0.0], [math.inf, 0.0, 0.0]]),
}


def _spec(fs=FS, num_taps=64, l_min=0, fc=3.5e9, t0=0.0, dt=0.0, num_times=1,
          parts=abi.CHANNEL_LOS | abi.CHANNEL_SCATTER):
    return abi.taps_spec(fs, num_taps, l_min, fc, t0, dt, num_times, parts=parts)


def _arrays(re, te, fa):
    re = np.asarray(re, np.float32).reshape(-1, 3)
    te = np.asarray(te, np.float32).reshape(-1, 3)
    # host buffers stand in for device pointers: a refused call never reads them
    keep = (np.ascontiguousarray(re), np.ascontiguousarray(te))
    a = abi.ArraySpec(re.shape[0], te.shape[0], keep[0].ctypes.data if re.size else 8,
                      keep[1].ctypes.data if te.size else 8, fa)
    return a, keep


def _have_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.parametrize("bad", sorted(BAD_CALLS))
def test_invalid_call_is_refused_by_the_device_entries(product_lib, bad):
    over, re, te, fa, what = BAD_CALLS[bad]
    spec = _spec(**over)
    arr, _keep = _arrays(re, te, fa)
    out = C.c_uint64(7)
    assert product_lib.hrt_array_taps_scratch_bytes(None, None, C.byref(spec), C.byref(arr), C.byref(out)) \
        == HRT_E_INVALID
    assert out.value == 7
    err = product_lib.hrt_last_error()
    assert err.startswith(b"hrt_array_taps: ") and what.encode() in err, err
    assert product_lib.hrt_array_taps(None, None, None, C.byref(spec), C.byref(arr), None, 0, None, 0, None) \
        == HRT_E_INVALID
    assert product_lib.hrt_last_error() == err


@pytest.mark.parametrize("bad", sorted(BAD_CALLS) + sorted(BAD_OFFSETS))
def test_invalid_call_is_refused_by_the_drop_in(product_lib, bad):
    """the C drop-in refuses it before it creates a problem (no device needed to get the answer)"""
    if bad in BAD_CALLS:
        over, re, te, fa, what = BAD_CALLS[bad]
    else:
        (re, te), over, fa, what = BAD_OFFSETS[bad], {}, 3e9, "finite"
    with pytest.raises(RuntimeError, match=r"hrt_compute_array_taps failed \(-1\): hrt_array_taps: ") as e:
        abi.run_compute_array_taps(product_lib, *K.args(K.small(K.C1, 64)), _spec(**over), re, te,
                                   array_frequency=fa)
    assert what in str(e.value)


def test_null_spec_and_arrays_are_refused(product_lib):
    spec = _spec()
    arr, _keep = _arrays(ONE, ONE, 3e9)
    assert product_lib.hrt_array_taps_scratch_bytes(None, None, None, C.byref(arr), None) == HRT_E_INVALID
    assert product_lib.hrt_last_error() == b"hrt_array_taps: NULL spec"
    assert product_lib.hrt_array_taps_scratch_bytes(None, None, C.byref(spec), None, None) == HRT_E_INVALID
    assert product_lib.hrt_last_error() == b"hrt_array_taps: NULL arrays"
    arr = abi.ArraySpec(1, 1, None, None, 3e9)
    assert product_lib.hrt_array_taps_scratch_bytes(None, None, C.byref(spec), C.byref(arr), None) \
        == HRT_E_INVALID
    assert product_lib.hrt_last_error() == b"hrt_array_taps: NULL element offsets"
    arr, _keep = _arrays(ONE, ONE, 3e9)
    assert product_lib.hrt_array_taps(None, None, None, C.byref(spec), C.byref(arr), None, 0, None, 0, None) \
        == HRT_E_INVALID
    assert product_lib.hrt_last_error() == b"hrt_array_taps: NULL argument"


def test_largest_grid_and_tap_range_pass_the_checks(product_lib):
    """Nr * Nt * T * L = 2^24, T * L = 2^20, 1024 elements a side and taps reaching +-2^24 are accepted (what fails
    without a problem is the NULL problem); one point more is refused"""
    ok = [(dict(num_taps=1 << 12, num_times=1 << 6), (4, 3), (16, 3)),
          (dict(num_taps=1 << 10, num_times=1 << 10), (4, 3), (4, 3)),
          (dict(num_taps=1 << 20), (4, 3), (4, 3)),
          (dict(num_taps=16), (1024, 3), (1024, 3)),
          (dict(l_min=-(1 << 24), num_taps=64), (2, 3), (2, 3)),
          (dict(l_min=(1 << 24) - 64, num_taps=64), (2, 3), (2, 3)),
          (dict(fc=0.0, parts=abi.CHANNEL_LOS), (1, 3), (1, 3))]
    for over, rs, ts in ok:
        spec = _spec(**over)
        arr, _keep = _arrays(np.zeros(rs), np.zeros(ts), 3e9)
        assert product_lib.hrt_array_taps_scratch_bytes(None, None, C.byref(spec), C.byref(arr), None) \
            == HRT_E_INVALID
        assert product_lib.hrt_last_error() == b"hrt_array_taps: NULL argument", over
    spec = _spec(num_taps=(1 << 12) + 1, num_times=1 << 6)
    arr, _keep = _arrays(np.zeros((4, 3)), np.zeros((16, 3)), 3e9)
    assert product_lib.hrt_array_taps_scratch_bytes(None, None, C.byref(spec), C.byref(arr), None) == HRT_E_INVALID
    assert product_lib.hrt_last_error() == \
        b"hrt_array_taps: Nr * Nt * num_times * num_taps = %d > 2^24" % (64 * 64 * ((1 << 12) + 1))


def test_existing_entries_keep_their_messages(product_lib):
    """the checks the new entry shares: the taps and array channel entries still name themselves"""
    spec = _spec(num_taps=0)
    assert product_lib.hrt_taps_scratch_bytes(None, None, C.byref(spec), None) == HRT_E_INVALID
    assert product_lib.hrt_last_error() == b"hrt_taps: num_taps and num_times must be > 0"
    ch = abi.channel_spec(3.5e9, 30e3, 1 << 10, num_times=1 << 10)
    arr, _keep = _arrays(ULA2, np.zeros((9, 3)), 3e9)
    assert product_lib.hrt_array_channel_scratch_bytes(None, None, C.byref(ch), C.byref(arr), None) == HRT_E_INVALID
    assert product_lib.hrt_last_error() == b"hrt_array_channel: Nr * Nt * num_times * num_freqs = 18874368 > 2^24"


def _pybind():
    import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    return hermespy_rt


# (pybind forms parts from los / scatter: it has no unknown bits to pass)
@pytest.mark.parametrize("bad", sorted(set(BAD_CALLS) - {"unknown_part"}) + sorted(BAD_OFFSETS))
def test_pybind_refuses_invalid_call(bad):
    hermespy_rt = _pybind()
    if bad in BAD_CALLS:
        over, re, te, fa, what = BAD_CALLS[bad]
    else:
        (re, te), over, fa, what = BAD_OFFSETS[bad], {}, 3e9, "finite"
    c = K.small(K.C1, 64)
    args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], 1, 1, 64, 1)
    kw = dict(fs=FS, num_taps=64)
    kw.update({k: v for k, v in over.items() if k != "parts"})
    names = {"fs": "sampling_rate", "fc": "center_frequency"}
    kw = {names.get(k, k): v for k, v in kw.items()}
    if over.get("parts") == 0:
        kw.update(los=False, scatter=False)
    with pytest.raises(ValueError, match="compute_array_taps: hrt_array_taps: ") as e:
        hermespy_rt.compute_array_taps(*args, kw.pop("sampling_rate"), kw.pop("num_taps"),
                                       np.asarray(re, np.float32), np.asarray(te, np.float32),
                                       array_frequency=fa, **kw)
    assert what in str(e.value)


def test_pybind_defaults_and_shapes():
    """center_frequency and array_frequency default to the carrier; a bad element shape is refused"""
    hermespy_rt = _pybind()
    c = K.small(K.C1, 64)
    args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], 1, 1, 64, 1)
    el = np.zeros((1, 3), np.float32)
    with pytest.raises(ValueError, match="2\\^24"):   # the limit, not a frequency, refuses this one
        hermespy_rt.compute_array_taps(*args, FS, 1 << 20, el, np.zeros((32, 3), np.float32))
    with pytest.raises(ValueError, match="shape"):
        hermespy_rt.compute_array_taps(*args, FS, 16, np.zeros(4, np.float32), el)


def test_export_list_covers_the_array_taps_entries():
    names = ("hrt_array_taps_scratch_bytes", "hrt_array_taps", "hrt_compute_array_taps")
    for n in names:
        assert n in lib.EXPORTED
    exports = open(os.path.join(REPO, "hermespy-rt_amd", "csrc", "exports.map")).read()
    headers = "".join(open(os.path.join(REPO, "include", h)).read() for h in ("hermespy_rt.h", "hrt_device.h"))
    for n in names:
        assert n + ";" in exports and n + "(" in headers


def test_compute_array_taps_without_device_fails_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny call
    succeeds and returns finite taps of the array layout.)"""
    c = K.small(K.C1, 64)
    if _have_gpu():
        h = abi.run_compute_array_taps(product_lib, *K.args(c), _spec(num_taps=16, num_times=2), ULA2, ONE)
        assert h.shape == (1, 1, 2, 1, 2, 2, 16) and np.isfinite(h.view(np.float32)).all()
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_array_taps failed \(-3\)") as e:
        abi.run_compute_array_taps(product_lib, *K.args(c), _spec(num_taps=16, num_times=2), ULA2, ONE)
    assert "HIP" in str(e.value)
