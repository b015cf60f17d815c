"""Argument checks of the taps entries (hrt_taps_scratch_bytes, hrt_taps, hrt_compute_taps, hermespy_rt.compute_taps):
a refused spec returns HRT_E_INVALID before the device is touched, so these run without a GPU.  Without a device a
valid call fails loudly (HRT_E_HIP), never with a CPU result."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi

from . import configs as K

HRT_E_INVALID, HRT_E_HIP = -1, -3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 122.88e6

# name -> (spec overrides, what the message names)
BAD_SPECS = {
    "no_taps": (dict(num_taps=0), "num_taps"),
    "no_times": (dict(num_times=0), "num_times"),
    "too_many_points": (dict(num_taps=1 << 10, num_times=(1 << 10) + 1), "2^20"),
    "taps_over_2_20": (dict(num_taps=(1 << 20) + 1), "2^20"),
    "fs_zero": (dict(fs=0.0), "sampling rate"),
    "fs_negative": (dict(fs=-FS), "sampling rate"),
    "fs_nan": (dict(fs=math.nan), "sampling rate"),
    "fs_inf": (dict(fs=math.inf), "sampling rate"),
    "fc_nan": (dict(fc=math.nan), "finite"),
    "t0_inf": (dict(t0=math.inf), "finite"),
    "dt_nan": (dict(dt=-math.nan), "finite"),
    "l_min_below": (dict(l_min=-(1 << 24) - 1), "2^24"),
    "l_min_above": (dict(l_min=(1 << 24) + 1), "2^24"),
    "last_tap_above": (dict(l_min=(1 << 24) - 63, num_taps=64), "2^24"),
    "no_parts": (dict(parts=0), "parts"),
    "unknown_part": (dict(parts=abi.CHANNEL_SCATTER | 8), "parts"),
}


def _spec(fs=FS, num_taps=64, l_min=0, fc=3.5e9, t0=0.0, dt=0.0, num_times=1,
          parts=abi.CHANNEL_LOS | abi.CHANNEL_SCATTER):
    return abi.taps_spec(fs, num_taps, l_min, fc, t0, dt, num_times, parts=parts)


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def test_taps_spec_struct_matches_c(tmp_path):
    fields = ["fs_hz", "fc_hz", "t0_s", "dt_s", "l_min", "num_taps", "num_times", "parts"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hrt_device.h"\n'
                    'int main(void){printf("%zu' + ' %zu' * len(fields) + '\\n", sizeof(hrt_taps_spec)' +
                    "".join(", offsetof(hrt_taps_spec, %s)" % f for f in fields) + ');return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = abi.TapsSpec
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]


@pytest.mark.parametrize("bad", sorted(BAD_SPECS))
def test_invalid_spec_is_refused_by_every_entry(product_lib, bad):
    over, what = BAD_SPECS[bad]
    spec = _spec(**over)
    out = C.c_uint64(7)
    assert product_lib.hrt_taps_scratch_bytes(None, None, C.byref(spec), C.byref(out)) == HRT_E_INVALID
    assert out.value == 7
    assert what.encode() in product_lib.hrt_last_error()
    assert product_lib.hrt_taps(None, None, None, C.byref(spec), None, 0, None, 0, None) == HRT_E_INVALID
    assert b"hrt_taps" in product_lib.hrt_last_error()
    # the drop-in entry refuses it before it creates a problem (no device needed to get the answer)
    with pytest.raises(RuntimeError, match=r"hrt_compute_taps failed \(-1\)"):
        abi.run_compute_taps(product_lib, *K.args(K.small(K.C1, 64)), spec)
    assert what.encode() in product_lib.hrt_last_error()


def test_largest_grid_and_tap_range_pass_the_spec_check(product_lib):
    """L * T = 2^20 and taps reaching +-2^24 pass the spec check (what fails without a problem is the NULL
    problem)"""
    for over in (dict(num_taps=1 << 10, num_times=1 << 10), dict(num_taps=1 << 20),
                 dict(l_min=-(1 << 24), num_taps=64), dict(l_min=(1 << 24) - 64, num_taps=64),
                 dict(fc=0.0, parts=abi.CHANNEL_LOS), dict(fs=1e-3, parts=abi.CHANNEL_SCATTER)):
        spec = _spec(**over)
        assert product_lib.hrt_taps_scratch_bytes(None, None, C.byref(spec), None) == HRT_E_INVALID
        assert b"NULL" in product_lib.hrt_last_error(), over


def _pybind():
    import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    return hermespy_rt


PYBIND_BAD = {
    "no_taps": (dict(num_taps=0), "num_taps"),
    "too_many_points": (dict(num_taps=1 << 20, num_times=2), "2\\^20"),
    "fs_zero": (dict(sampling_rate=0.0), "sampling rate"),
    "fs_nan": (dict(sampling_rate=math.nan), "sampling rate"),
    "fc_inf": (dict(center_frequency=math.inf), "finite"),
    "dt_nan": (dict(dt=math.nan), "finite"),
    "l_min_below": (dict(l_min=-(1 << 24) - 1), "2\\^24"),
    "last_tap_above": (dict(l_min=(1 << 24), num_taps=1), "2\\^24"),
    "no_parts": (dict(los=False, scatter=False), "parts"),
}


@pytest.mark.parametrize("bad", sorted(PYBIND_BAD))
def test_pybind_refuses_invalid_spec(bad):
    hermespy_rt = _pybind()
    c = K.small(K.C1, 64)
    args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], 1, 1, 64, 1)
    kw = dict(sampling_rate=FS, num_taps=64)
    over, what = PYBIND_BAD[bad]
    kw.update(over)
    with pytest.raises(ValueError, match=what):
        hermespy_rt.compute_taps(*args, **kw)


def test_compute_taps_without_device_fails_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny call
    succeeds and returns finite taps.)"""
    c = K.small(K.C1, 64)
    if _have_gpu():
        h = abi.run_compute_taps(product_lib, *K.args(c), _spec(num_taps=16))
        assert h.shape == (1, 1, 2, 1, 16) and np.isfinite(h.view(np.float32)).all()
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_taps failed \(-3\)") as e:
        abi.run_compute_taps(product_lib, *K.args(c), _spec(num_taps=16))
    assert "HIP" in str(e.value)
