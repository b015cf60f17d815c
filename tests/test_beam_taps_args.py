"""Argument checks of the beamformed taps entries (hrt_beam_taps_scratch_bytes, hrt_beam_taps, hrt_compute_beam_taps,
hermespy_rt.compute_beam_taps, Tracer.beam_taps' host checks): a refused call returns HRT_E_INVALID before the device
is touched, so these run without a GPU.  Without a device a valid call fails loudly (HRT_E_HIP), never with a CPU
result."""
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

ONE = [[0.0, 0.0, 0.0]]
ULA2 = [[0.0, 0.0, 0.0], [0.0, 0.05, 0.0]]


def _w(beams, elements):
    return np.full((beams, elements), 0.5 - 0.25j, np.complex64)


# name -> (spec overrides, rx_elements, tx_elements, Br, Bt, array frequency, what the message names)
BAD_CALLS = {
    "no_rx_elements": ({}, np.zeros((0, 3)), ONE, 1, 1, 3e9, "elements"),
    "no_tx_elements": ({}, ONE, np.zeros((0, 3)), 1, 1, 3e9, "elements"),
    "rx_257": ({}, np.zeros((257, 3)), ONE, 1, 1, 3e9, "elements"),
    "tx_257": ({}, ONE, np.zeros((257, 3)), 1, 1, 3e9, "elements"),
    "no_rx_beams": ({}, ONE, ULA2, 0, 1, 3e9, "beams"),
    "no_tx_beams": ({}, ULA2, ONE, 1, 0, 3e9, "beams"),
    "rx_beams_257": ({"num_taps": 1}, ONE, ONE, 257, 1, 3e9, "beams"),
    "tx_beams_257": ({"num_taps": 1}, ONE, ONE, 1, 257, 3e9, "beams"),
    "over_2_24": ({"num_taps": 1 << 10, "num_times": 1 << 10}, ONE, ONE, 2, 9, 3e9, "2^24"),
    "just_over_2_24": ({"num_taps": (1 << 12) + 1, "num_times": 1 << 6}, ONE, ONE, 8, 8, 3e9, "2^24"),
    "fa_zero": ({}, ONE, ONE, 1, 1, 0.0, "array frequency"),
    "fa_negative": ({}, ONE, ONE, 1, 1, -3e9, "array frequency"),
    "fa_nan": ({}, ONE, ONE, 1, 1, math.nan, "array frequency"),
    "fa_inf": ({}, ONE, ONE, 1, 1, math.inf, "array frequency"),
    # every hrt_taps_spec check
    "spec_no_taps": ({"num_taps": 0}, ONE, ONE, 1, 1, 3e9, "num_taps"),
    "spec_no_times": ({"num_times": 0}, ONE, ONE, 1, 1, 3e9, "num_times"),
    "spec_over_2_20": ({"num_taps": 1 << 11, "num_times": (1 << 9) + 1}, ONE, ONE, 1, 1, 3e9, "2^20"),
    "spec_fs_zero": ({"fs": 0.0}, ONE, ONE, 1, 1, 3e9, "sampling rate"),
    "spec_fs_negative": ({"fs": -1e6}, ONE, ONE, 1, 1, 3e9, "sampling rate"),
    "spec_fs_nan": ({"fs": math.nan}, ONE, ONE, 1, 1, 3e9, "sampling rate"),
    "spec_fc_inf": ({"fc": math.inf}, ONE, ONE, 1, 1, 3e9, "finite"),
    "spec_t0_nan": ({"t0": math.nan}, ONE, ONE, 1, 1, 3e9, "finite"),
    "spec_dt_inf": ({"dt": math.inf}, ONE, ONE, 1, 1, 3e9, "finite"),
    "spec_l_min_low": ({"l_min": -(1 << 24) - 1}, ONE, ONE, 1, 1, 3e9, "tap indices"),
    "spec_l_max_high": ({"l_min": (1 << 24) - 63}, ONE, ONE, 1, 1, 3e9, "tap indices"),
    "spec_no_parts": ({"parts": 0}, ONE, ONE, 1, 1, 3e9, "parts"),
}
# offsets and weights are checked where they are host memory (the C drop-in, pybind, Tracer), not in the device entry:
# name -> (rx_elements, tx_elements, W_rx, W_tx, what the message names)
BAD_HOST = {
    "rx_offset_nan": ([[0.0, math.nan, 0.0]], ONE, _w(1, 1), _w(1, 1), "element"),
    "tx_offset_inf": (ONE, [[0.0, 0.0, 0.0], [math.inf, 0.0, 0.0]], _w(1, 1), _w(2, 2), "element"),
    "rx_weight_nan": (ULA2, ONE, np.array([[1.0, complex(0.0, math.nan)]], np.complex64), _w(1, 1), "RX weight"),
    "tx_weight_inf": (ONE, ULA2, _w(1, 1), np.array([[1.0, 2.0], [math.inf, 0.0]], np.complex64), "TX weight"),
}


def _spec(num_taps=64, num_times=1, fs=122.88e6, fc=3.5e9, l_min=0, t0=0.0, dt=0.0,
          parts=abi.CHANNEL_LOS | abi.CHANNEL_SCATTER):
    return abi.taps_spec(fs, num_taps, l_min, fc, t0, dt, num_times, parts=parts)


def _specs(re, te, br, bt, fa):
    """(ArraySpec, BeamSpec, what keeps their buffers alive): host buffers stand in for device pointers, a refused
    call never reads them"""
    re = np.ascontiguousarray(np.asarray(re, np.float32).reshape(-1, 3))
    te = np.ascontiguousarray(np.asarray(te, np.float32).reshape(-1, 3))
    wr, wt = _w(br, re.shape[0]), _w(bt, te.shape[0])
    a = abi.ArraySpec(re.shape[0], te.shape[0], re.ctypes.data if re.size else 8, te.ctypes.data if te.size else 8, fa)
    b = abi.BeamSpec(br, bt, wr.ctypes.data if wr.size else 8, wt.ctypes.data if wt.size else 8)
    return a, b, (re, te, wr, wt)


def _have_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.parametrize("bad", sorted(BAD_CALLS))
def test_invalid_call_is_refused_by_the_device_entries(product_lib, bad):
    over, re, te, br, bt, fa, what = BAD_CALLS[bad]
    spec = _spec(**over)
    arr, bm, _keep = _specs(re, te, br, bt, fa)
    out = C.c_uint64(7)
    assert product_lib.hrt_beam_taps_scratch_bytes(None, None, C.byref(spec), C.byref(arr), C.byref(bm),
                                                   C.byref(out)) == HRT_E_INVALID
    assert out.value == 7
    assert what.encode() in product_lib.hrt_last_error()
    assert product_lib.hrt_beam_taps(None, None, None, C.byref(spec), C.byref(arr), C.byref(bm), None, 0, None, 0,
                                     None) == HRT_E_INVALID
    assert what.encode() in product_lib.hrt_last_error() and b"hrt_beam_taps" in product_lib.hrt_last_error()


def _host_case(bad):
    """-> spec overrides, rx_elements, tx_elements, W_rx, W_tx, array frequency, what"""
    if bad in BAD_CALLS:
        over, re, te, br, bt, fa, what = BAD_CALLS[bad]
        nr, nt = np.asarray(re).reshape(-1, 3).shape[0], np.asarray(te).reshape(-1, 3).shape[0]
        return over, re, te, _w(br, nr), _w(bt, nt), fa, what
    re, te, wr, wt, what = BAD_HOST[bad]
    return {}, re, te, wr, wt, 3e9, what


@pytest.mark.parametrize("bad", sorted(BAD_CALLS) + sorted(BAD_HOST))
def test_invalid_call_is_refused_by_the_drop_in(product_lib, bad):
    """the C drop-in refuses it before it creates a problem (no device needed to get the answer)"""
    over, re, te, wr, wt, fa, what = _host_case(bad)
    with pytest.raises(RuntimeError, match=r"hrt_compute_beam_taps failed \(-1\)") as e:
        abi.run_compute_beam_taps(product_lib, *K.args(K.small(K.C1, 64)), _spec(**over), re, te, wr, wt,
                                  array_frequency=fa)
    assert what in str(e.value)


def test_null_pointers_are_refused(product_lib):
    spec = _spec()
    arr, bm, _keep = _specs(ONE, ONE, 1, 1, 3e9)
    q = product_lib.hrt_beam_taps_scratch_bytes
    assert q(None, None, None, C.byref(arr), C.byref(bm), None) == HRT_E_INVALID
    assert b"NULL spec" in product_lib.hrt_last_error()
    assert q(None, None, C.byref(spec), None, C.byref(bm), None) == HRT_E_INVALID
    assert b"NULL arrays" in product_lib.hrt_last_error()
    assert q(None, None, C.byref(spec), C.byref(arr), None, None) == HRT_E_INVALID
    assert b"NULL beams" in product_lib.hrt_last_error()
    no_el = abi.ArraySpec(1, 1, None, None, 3e9)
    assert q(None, None, C.byref(spec), C.byref(no_el), C.byref(bm), None) == HRT_E_INVALID
    assert b"NULL element" in product_lib.hrt_last_error()
    for no_w in (abi.BeamSpec(1, 1, None, bm.tx_weights), abi.BeamSpec(1, 1, bm.rx_weights, None)):
        assert q(None, None, C.byref(spec), C.byref(arr), C.byref(no_w), None) == HRT_E_INVALID
        assert b"NULL beam weights" in product_lib.hrt_last_error()
    # a valid call with no problem / no output pointer
    assert q(None, None, C.byref(spec), C.byref(arr), C.byref(bm), None) == HRT_E_INVALID
    assert b"NULL argument" in product_lib.hrt_last_error()
    # the drop-in: NULL weights, NULL scene, NULL output
    f32p = C.POINTER(C.c_float)
    el = (abi.Vec3 * 1)()
    w = (C.c_float * 2)(1.0, 0.0)
    out = (C.c_float * 2 * 2 * 64)()
    call = lambda scene, wr, wt, o: product_lib.hrt_compute_beam_taps(   # noqa: E731
        scene, el, el, el, el, C.c_float(3.5), 1, 1, 64, 1, C.byref(spec), el, 1, el, 1, C.c_double(3e9), wr, 1, wt, 1,
        o, None)
    scene = abi.Scene()
    assert call(C.byref(scene), None, C.cast(w, f32p), C.cast(out, f32p)) == HRT_E_INVALID
    assert b"NULL beam weights" in product_lib.hrt_last_error()
    assert call(None, C.cast(w, f32p), C.cast(w, f32p), C.cast(out, f32p)) == HRT_E_INVALID
    assert b"NULL argument" in product_lib.hrt_last_error()
    assert call(C.byref(scene), C.cast(w, f32p), C.cast(w, f32p), None) == HRT_E_INVALID
    assert b"NULL argument" in product_lib.hrt_last_error()


def _accepted(product_lib, spec, arr, bm):
    """the checks pass: what fails without a problem is the NULL problem"""
    assert product_lib.hrt_beam_taps_scratch_bytes(None, None, C.byref(spec), C.byref(arr), C.byref(bm), None) \
        == HRT_E_INVALID
    return b"NULL argument" in product_lib.hrt_last_error()


def test_largest_sizes_pass_the_check(product_lib):
    """Br * Bt * T * L = 2^24 and 256 elements and beams a side are accepted; one tap more is refused"""
    arr, bm, _keep = _specs(np.zeros((8, 3)), np.zeros((8, 3)), 8, 8, 3e9)
    assert _accepted(product_lib, _spec(num_taps=1 << 12, num_times=1 << 6), arr, bm)
    assert not _accepted(product_lib, _spec(num_taps=(1 << 12) + 1, num_times=1 << 6), arr, bm)
    assert b"2^24" in product_lib.hrt_last_error()
    arr, bm, _keep = _specs(np.zeros((256, 3)), np.zeros((256, 3)), 256, 256, 3e9)
    assert _accepted(product_lib, _spec(num_taps=256), arr, bm)
    assert not _accepted(product_lib, _spec(num_taps=257), arr, bm)


def test_large_arrays_with_few_beams_pass_where_the_array_taps_are_refused(product_lib):
    """16 x 16 elements a side at L = 512: 2^25 element-domain points are refused by hrt_array_taps; with 8 x 8 beams
    the same elements are a 2^15-point problem here (there is no limit on Nr * Nt)"""
    spec = _spec(num_taps=512)
    arr, bm, _keep = _specs(np.zeros((256, 3)), np.zeros((256, 3)), 8, 8, 3e9)
    assert product_lib.hrt_array_taps_scratch_bytes(None, None, C.byref(spec), C.byref(arr), None) == HRT_E_INVALID
    assert b"2^24" in product_lib.hrt_last_error()
    assert _accepted(product_lib, spec, arr, bm)


def _pybind():
    import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    return hermespy_rt


def _pybind_args():
    c = K.small(K.C1, 64)
    return (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], 1, 1, 64, 1)


@pytest.mark.parametrize("bad", sorted(BAD_CALLS) + sorted(BAD_HOST))
def test_pybind_refuses_invalid_call(bad):
    hermespy_rt = _pybind()
    over, re, te, wr, wt, fa, what = _host_case(bad)
    kw = dict(num_taps=64, fs=122.88e6, num_times=1, los=True, scatter=True, center_frequency=3.5e9)
    names = {"fc": "center_frequency"}
    kw.update({names.get(k, k): v for k, v in over.items() if k != "parts"})
    if over.get("parts") == 0:
        kw.update(los=False, scatter=False)
    with pytest.raises(ValueError, match="compute_beam_taps") as e:
        hermespy_rt.compute_beam_taps(*_pybind_args(), kw.pop("fs"), kw.pop("num_taps"),
                                      np.asarray(re, np.float32).reshape(-1, 3),
                                      np.asarray(te, np.float32).reshape(-1, 3), wr, wt, array_frequency=fa, **kw)
    assert what in str(e.value)


def test_pybind_refuses_weights_of_the_wrong_shape_or_dtype():
    hermespy_rt = _pybind()
    el2, el1 = np.asarray(ULA2, np.float32), np.asarray(ONE, np.float32)
    call = lambda wr, wt: hermespy_rt.compute_beam_taps(*_pybind_args(), 122.88e6, 16, el2, el1, wr, wt)  # noqa: E731
    with pytest.raises(ValueError, match="rx_weights"):
        call(_w(3, 3), _w(1, 1))                          # 3 weights a beam for 2 elements
    with pytest.raises(ValueError, match="rx_weights"):
        call(_w(1, 2).reshape(2), _w(1, 1))               # not (beams, elements)
    with pytest.raises(ValueError, match="rx_weights"):
        call(_w(1, 2).astype(np.complex128), _w(1, 1))    # not complex64
    with pytest.raises(ValueError, match="tx_weights"):
        call(_w(1, 2), np.ones((1, 1), np.float32))       # real
    with pytest.raises(ValueError, match="tx_weights"):
        call(_w(1, 2), _w(2, 2))
    with pytest.raises(ValueError, match="2\\^24"):   # the limit, not the shapes, refuses this one
        hermespy_rt.compute_beam_taps(*_pybind_args(), 122.88e6, 1 << 20, el2, el1, _w(32, 2), _w(1, 1))


class _NoDevice:
    """what Tracer.beam_taps reads before it reaches the device: its host checks run on this stand-in"""
    f_ghz = 3.5

    def __getattr__(self, name):
        raise AssertionError("Tracer.beam_taps reached for %r before its host checks refused the call" % name)


@pytest.mark.parametrize("bad", sorted(BAD_HOST) + ["wrong_shape", "integer_weights"])
def test_tracer_refuses_bad_host_arrays_before_the_device(bad):
    """Tracer.beam_taps refuses non-finite offsets and weights, and weights of the wrong shape or kind, with ValueError
    before it touches the library or the device (everything else is the device entry's to refuse: the cases above)"""
    from hermespy_rt_amd.device import Tracer
    if bad in BAD_HOST:
        re, te, wr, wt, _ = BAD_HOST[bad]
    elif bad == "wrong_shape":
        re, te, wr, wt = ULA2, ONE, _w(2, 3), _w(1, 1)
    else:
        re, te, wr, wt = ULA2, ONE, np.ones((1, 2), np.int32), _w(1, 1)
    tr = _NoDevice()
    tr._elements = lambda *a: Tracer._elements(tr, *a)
    with pytest.raises(ValueError):
        Tracer.beam_taps(tr, re, te, wr, wt, 122.88e6, 16)


def test_export_list_covers_the_beam_taps_entries():
    names = ("hrt_beam_taps_scratch_bytes", "hrt_beam_taps", "hrt_compute_beam_taps")
    for n in names:
        assert n in lib.EXPORTED
    exports = open(os.path.join(REPO, "hermespy-rt_amd", "csrc", "exports.map")).read()
    headers = "".join(open(os.path.join(REPO, "include", h)).read() for h in ("hermespy_rt.h", "hrt_device.h"))
    for n in names:
        assert n + ";" in exports and n + "(" in headers


def test_compute_beam_taps_without_device_fails_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny call
    succeeds and returns finite taps of the beam layout.)"""
    c = K.small(K.C1, 64)
    if _have_gpu():
        h = abi.run_compute_beam_taps(product_lib, *K.args(c), _spec(num_taps=16), ULA2, ONE, _w(3, 2), _w(1, 1))
        assert h.shape == (1, 1, 3, 1, 2, 1, 16) and np.isfinite(h.view(np.float32)).all()
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_beam_taps failed \(-3\)") as e:
        abi.run_compute_beam_taps(product_lib, *K.args(c), _spec(num_taps=16), ULA2, ONE, _w(3, 2), _w(1, 1))
    assert "HIP" in str(e.value)
