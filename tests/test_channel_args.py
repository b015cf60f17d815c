"""Argument checks of the channel entries (hrt_channel_scratch_bytes, hrt_channel, hrt_compute_channel,
hermespy_rt.compute_channel): a refused spec returns HRT_E_INVALID before the device is touched, so these run
without a GPU.  Without a device a valid call fails loudly (HRT_E_HIP), never with a CPU result."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi, lib

from . import configs as K

HRT_E_INVALID, HRT_E_HIP = -1, -3

BAD_SPECS = {
    "no_freqs": dict(num_freqs=0),
    "no_times": dict(num_times=0),
    "too_many_points": dict(num_freqs=1 << 10, num_times=(1 << 10) + 1),
    "one_over_2_20": dict(num_freqs=(1 << 20) + 1, num_times=1),
    "no_parts": dict(parts=0),
    "unknown_part": dict(parts=abi.CHANNEL_LOS | 4),
    "f0_nan": dict(f0=math.nan),
    "df_inf": dict(df=math.inf),
    "t0_nan": dict(t0=math.nan),
    "dt_inf": dict(dt=-math.inf),
}


def _spec(num_freqs=64, num_times=1, f0=3.5e9, df=30e3, t0=0.0, dt=0.0, parts=abi.CHANNEL_LOS | abi.CHANNEL_SCATTER):
    return abi.channel_spec(f0, df, num_freqs, t0, dt, num_times, parts=parts)


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def test_spec_struct_matches_c(tmp_path):
    import subprocess
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hrt_device.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(hrt_channel_spec), '
                    'offsetof(hrt_channel_spec, t0_s), offsetof(hrt_channel_spec, num_times), '
                    'offsetof(hrt_channel_spec, parts));return 0;}\n')
    exe = tmp_path / "sz"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.check_call(["gcc", "-I", inc, str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = abi.ChannelSpec
    assert got == [C.sizeof(S), S.t0_s.offset, S.num_times.offset, S.parts.offset]


@pytest.mark.parametrize("bad", sorted(BAD_SPECS))
def test_invalid_spec_is_refused_by_every_entry(product_lib, bad):
    spec = _spec(**BAD_SPECS[bad])
    out = C.c_uint64(7)
    assert product_lib.hrt_channel_scratch_bytes(None, None, C.byref(spec), C.byref(out)) == HRT_E_INVALID
    assert out.value == 7
    assert product_lib.hrt_channel(None, None, None, C.byref(spec), None, 0, None, 0, None) == HRT_E_INVALID
    assert b"hrt_channel" in product_lib.hrt_last_error()
    # the drop-in entry refuses it before it creates a problem (no device needed to get the answer)
    with pytest.raises(RuntimeError, match=r"hrt_compute_channel failed \(-1\)"):
        abi.run_compute_channel(product_lib, *K.args(K.small(K.C1, 64)), spec)


def test_largest_grid_passes_the_spec_check(product_lib):
    """K * T = 2^20 is accepted by the spec check (what fails without a problem is the NULL problem)"""
    spec = _spec(num_freqs=1 << 10, num_times=1 << 10)
    assert product_lib.hrt_channel_scratch_bytes(None, None, C.byref(spec), None) == HRT_E_INVALID
    assert b"NULL" in product_lib.hrt_last_error()
    spec = _spec(num_freqs=(1 << 10) + 1, num_times=1 << 10)
    assert product_lib.hrt_channel_scratch_bytes(None, None, C.byref(spec), None) == HRT_E_INVALID
    assert b"2^20" in product_lib.hrt_last_error()


def test_pybind_refuses_invalid_spec():
    import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    c = K.small(K.C1, 64)
    args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], 1, 1, 64, 1)
    with pytest.raises(ValueError, match="2\\^20"):
        hermespy_rt.compute_channel(*args, 3e9, 30e3, 1 << 20, num_times=2)
    with pytest.raises(ValueError, match="parts"):
        hermespy_rt.compute_channel(*args, 3e9, 30e3, 16, los=False, scatter=False)
    with pytest.raises(ValueError, match="finite"):
        hermespy_rt.compute_channel(*args, math.nan, 30e3, 16)


def test_compute_channel_without_device_fails_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny
    call succeeds and returns a finite channel.)"""
    c = K.small(K.C1, 64)
    if _have_gpu():
        H = abi.run_compute_channel(product_lib, *K.args(c), _spec(num_freqs=16))
        assert H.shape == (1, 1, 2, 1, 16) and np.isfinite(H.view(np.float32)).all()
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_channel failed \(-3\)") as e:
        abi.run_compute_channel(product_lib, *K.args(c), _spec(num_freqs=16))
    assert "HIP" in str(e.value)
