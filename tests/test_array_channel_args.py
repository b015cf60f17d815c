"""Argument checks of the antenna-array channel entries (hrt_array_channel_scratch_bytes, hrt_array_channel,
hrt_compute_array_channel, hermespy_rt.compute_array_channel): a refused call returns HRT_E_INVALID before the
device is touched, so these run without a GPU.  Without a device a valid call fails loudly (HRT_E_HIP), never with
a CPU result."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi, lib

from . import configs as K

HRT_E_INVALID, HRT_E_HIP = -1, -3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ONE = [[0.0, 0.0, 0.0]]
ULA2 = [[0.0, 0.0, 0.0], [0.0, 0.05, 0.0]]

# name -> (spec overrides, rx_elements, tx_elements, array frequency, what the message names)
BAD_CALLS = {
    "no_rx_elements": ({}, np.zeros((0, 3)), ONE, 3e9, "elements"),
    "no_tx_elements": ({}, ONE, np.zeros((0, 3)), 3e9, "elements"),
    "rx_1025": ({}, np.zeros((1025, 3)), ONE, 3e9, "elements"),
    "tx_1025": ({"num_freqs": 1}, ONE, np.zeros((1025, 3)), 3e9, "elements"),
    "over_2_24": ({"num_freqs": 1 << 10, "num_times": 1 << 10}, ULA2, np.zeros((9, 3)), 3e9, "2^24"),
    "fa_zero": ({}, ONE, ONE, 0.0, "array frequency"),
    "fa_negative": ({}, ONE, ONE, -3e9, "array frequency"),
    "fa_nan": ({}, ONE, ONE, math.nan, "array frequency"),
    "fa_inf": ({}, ONE, ONE, math.inf, "array frequency"),
    "spec_no_freqs": ({"num_freqs": 0}, ONE, ONE, 3e9, "num_freqs"),
    "spec_no_parts": ({"parts": 0}, ONE, ONE, 3e9, "parts"),
    "spec_f0_nan": ({"f0": math.nan}, ONE, ONE, 3e9, "finite"),
}
# offsets are checked where they are host memory (the C drop-in, pybind, Tracer), not in the device entry
BAD_OFFSETS = {
    "rx_nan": ([[0.0, math.nan, 0.0]], ONE),
    "tx_inf": (ONE, [[0.0, 0.0, 0.0], [math.inf, 0.0, 0.0]]),
}


def _spec(num_freqs=64, num_times=1, f0=3.5e9, df=30e3, t0=0.0, dt=0.0, parts=abi.CHANNEL_LOS | abi.CHANNEL_SCATTER):
    return abi.channel_spec(f0, df, num_freqs, t0, dt, num_times, parts=parts)


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


def test_array_spec_struct_matches_c(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hrt_device.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(hrt_array_spec), '
                    'offsetof(hrt_array_spec, num_rx_elements), offsetof(hrt_array_spec, num_tx_elements), '
                    'offsetof(hrt_array_spec, rx_elements), offsetof(hrt_array_spec, tx_elements), '
                    'offsetof(hrt_array_spec, array_frequency_hz));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = abi.ArraySpec
    assert got == [C.sizeof(S), S.num_rx_elements.offset, S.num_tx_elements.offset, S.rx_elements.offset,
                   S.tx_elements.offset, S.array_frequency_hz.offset]


@pytest.mark.parametrize("bad", sorted(BAD_CALLS))
def test_invalid_call_is_refused_by_the_device_entries(product_lib, bad):
    over, re, te, fa, what = BAD_CALLS[bad]
    spec = _spec(**over)
    arr, _keep = _arrays(re, te, fa)
    out = C.c_uint64(7)
    assert product_lib.hrt_array_channel_scratch_bytes(None, None, C.byref(spec), C.byref(arr), C.byref(out)) \
        == HRT_E_INVALID
    assert out.value == 7
    assert what.encode() in product_lib.hrt_last_error()
    assert product_lib.hrt_array_channel(None, None, None, C.byref(spec), C.byref(arr), None, 0, None, 0, None) \
        == HRT_E_INVALID
    assert b"hrt_" in product_lib.hrt_last_error()


@pytest.mark.parametrize("bad", sorted(BAD_CALLS) + sorted(BAD_OFFSETS))
def test_invalid_call_is_refused_by_the_drop_in(product_lib, bad):
    """the C drop-in refuses it before it creates a problem (no device needed to get the answer)"""
    if bad in BAD_CALLS:
        over, re, te, fa, what = BAD_CALLS[bad]
    else:
        (re, te), over, fa, what = BAD_OFFSETS[bad], {}, 3e9, "finite"
    with pytest.raises(RuntimeError, match=r"hrt_compute_array_channel failed \(-1\)") as e:
        abi.run_compute_array_channel(product_lib, *K.args(K.small(K.C1, 64)), _spec(**over), re, te,
                                      array_frequency=fa)
    assert what in str(e.value)


def test_null_arrays_are_refused(product_lib):
    spec = _spec()
    assert product_lib.hrt_array_channel_scratch_bytes(None, None, C.byref(spec), None, None) == HRT_E_INVALID
    arr = abi.ArraySpec(1, 1, None, None, 3e9)
    assert product_lib.hrt_array_channel_scratch_bytes(None, None, C.byref(spec), C.byref(arr), None) \
        == HRT_E_INVALID
    assert b"NULL element" in product_lib.hrt_last_error()


def test_largest_grid_passes_the_array_check(product_lib):
    """Nr * Nt * T * K = 2^24 and 1024 elements a side are accepted (what fails without a problem is the NULL
    problem); one point more is refused"""
    spec = _spec(num_freqs=1 << 12, num_times=1 << 6)
    arr, _keep = _arrays(np.zeros((8, 3)), np.zeros((8, 3)), 3e9)
    assert product_lib.hrt_array_channel_scratch_bytes(None, None, C.byref(spec), C.byref(arr), None) \
        == HRT_E_INVALID
    assert b"NULL argument" in product_lib.hrt_last_error()
    spec = _spec(num_freqs=(1 << 12) + 1, num_times=1 << 6)
    assert product_lib.hrt_array_channel_scratch_bytes(None, None, C.byref(spec), C.byref(arr), None) \
        == HRT_E_INVALID
    assert b"2^24" in product_lib.hrt_last_error()
    arr, _keep = _arrays(np.zeros((1024, 3)), np.zeros((1024, 3)), 3e9)
    spec = _spec(num_freqs=16)
    assert product_lib.hrt_array_channel_scratch_bytes(None, None, C.byref(spec), C.byref(arr), None) \
        == HRT_E_INVALID
    assert b"NULL argument" in product_lib.hrt_last_error()


def _pybind():
    import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    return hermespy_rt


@pytest.mark.parametrize("bad", sorted(BAD_CALLS) + sorted(BAD_OFFSETS))
def test_pybind_refuses_invalid_call(bad):
    hermespy_rt = _pybind()
    if bad in BAD_CALLS:
        over, re, te, fa, what = BAD_CALLS[bad]
    else:
        (re, te), over, fa, what = BAD_OFFSETS[bad], {}, 3e9, "finite"
    c = K.small(K.C1, 64)
    args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], 1, 1, 64, 1)
    kw = dict(num_freqs=64, f0=3.5e9, df=30e3, num_times=1, los=True, scatter=True)
    kw.update({k: v for k, v in over.items() if k != "parts"})
    if over.get("parts") == 0:
        kw.update(los=False, scatter=False)
    with pytest.raises(ValueError, match="compute_array_channel") as e:
        hermespy_rt.compute_array_channel(*args, kw.pop("f0"), kw.pop("df"), kw.pop("num_freqs"),
                                          np.asarray(re, np.float32), np.asarray(te, np.float32),
                                          array_frequency=fa, **kw)
    assert what in str(e.value)


def test_pybind_array_frequency_defaults_to_the_carrier():
    """array_frequency=None is accepted (the carrier); a bad one is refused like the C entry"""
    hermespy_rt = _pybind()
    c = K.small(K.C1, 64)
    args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], 1, 1, 64, 1)
    el = np.zeros((1, 3), np.float32)
    with pytest.raises(ValueError, match="2\\^24"):   # the limit, not the array frequency, refuses this one
        hermespy_rt.compute_array_channel(*args, 3e9, 30e3, 1 << 20, el, np.zeros((32, 3), np.float32))
    with pytest.raises(ValueError, match="shape"):
        hermespy_rt.compute_array_channel(*args, 3e9, 30e3, 16, np.zeros(4, np.float32), el)


def test_export_list_covers_the_array_entries():
    names = ("hrt_array_channel_scratch_bytes", "hrt_array_channel", "hrt_compute_array_channel")
    for n in names:
        assert n in lib.EXPORTED
    exports = open(os.path.join(REPO, "hermespy-rt_amd", "csrc", "exports.map")).read()
    headers = "".join(open(os.path.join(REPO, "include", h)).read() for h in ("hermespy_rt.h", "hrt_device.h"))
    for n in names:
        assert n + ";" in exports and n + "(" in headers


def test_compute_array_channel_without_device_fails_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny
    call succeeds and returns a finite channel of the array layout.)"""
    c = K.small(K.C1, 64)
    if _have_gpu():
        H = abi.run_compute_array_channel(product_lib, *K.args(c), _spec(num_freqs=16), ULA2, ONE)
        assert H.shape == (1, 1, 2, 1, 2, 1, 16) and np.isfinite(H.view(np.float32)).all()
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_array_channel failed \(-3\)") as e:
        abi.run_compute_array_channel(product_lib, *K.args(c), _spec(num_freqs=16), ULA2, ONE)
    assert "HIP" in str(e.value)
