"""Argument checks of the power entries (hrt_power_profiles_scratch_bytes, hrt_power_profiles,
hrt_compute_power_profiles, hermespy_rt.compute_power_profiles): a refused spec returns HRT_E_INVALID before the device
is touched, so these run without a GPU.  Without a device a valid call fails loudly (HRT_E_HIP), never with a CPU
result."""
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

# name -> (spec overrides, what the message names)
BAD_SPECS = {
    "no_parts": (dict(parts=0), "parts"),
    "unknown_part": (dict(parts=abi.CHANNEL_SCATTER | 4), "parts"),
    "delay_bins_over_2_16": (dict(num_delay_bins=(1 << 16) + 1), "num_delay_bins"),
    "tau0_nan": (dict(tau0=math.nan), "tau0"),
    "tau0_inf": (dict(tau0=-math.inf), "tau0"),
    "dtau_zero": (dict(dtau=0.0), "dtau"),
    "dtau_negative": (dict(dtau=-1e-9), "dtau"),
    "dtau_nan": (dict(dtau=math.nan), "dtau"),
    "dtau_inf": (dict(dtau=math.inf), "dtau"),
    "zenith_only": (dict(num_zenith_bins=4, num_azimuth_bins=0), "num_azimuth_bins"),
    "azimuth_only": (dict(num_zenith_bins=0, num_azimuth_bins=4), "num_zenith_bins"),
    "angles_over_2_14": (dict(num_zenith_bins=129, num_azimuth_bins=128), "num_zenith_bins * num_azimuth_bins"),
}


def _spec(tau0=0.0, dtau=1e-9, num_delay_bins=64, num_zenith_bins=0, num_azimuth_bins=0,
          parts=abi.CHANNEL_LOS | abi.CHANNEL_SCATTER):
    return abi.power_spec(tau0, dtau, num_delay_bins, num_zenith_bins, num_azimuth_bins, parts=parts)


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def test_power_spec_struct_matches_c(tmp_path):
    fields = ["tau0_s", "dtau_s", "num_delay_bins", "num_zenith_bins", "num_azimuth_bins", "parts"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hrt_device.h"\n'
                    'int main(void){printf("%zu' + ' %zu' * len(fields) + ' %d %d %d\\n", sizeof(hrt_power_spec)' +
                    "".join(", offsetof(hrt_power_spec, %s)" % f for f in fields) +
                    ', HRT_POWER_FIELDS, HRT_POWER_P_URX_X, HRT_POWER_P_LOS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = abi.PowerSpec
    assert got == ([C.sizeof(S)] + [getattr(S, f).offset for f in fields] +
                   [abi.POWER_FIELDS, abi.POWER_P_URX_X, abi.POWER_P_LOS])


def test_out_doubles(product_lib):
    for nrx, ntx, over in ((1, 1, {}), (3, 5, dict(num_zenith_bins=7, num_azimuth_bins=13)),
                           (2, 2, dict(num_delay_bins=0))):
        spec = _spec(**over)
        assert product_lib.hrt_power_out_doubles(nrx, ntx, C.byref(spec)) == abi.power_out_doubles(nrx, ntx, spec)
    assert product_lib.hrt_power_out_doubles(4, 4, None) == 0
    assert abi.power_out_doubles(1, 1, _spec(num_delay_bins=0)) == 2 * abi.POWER_FIELDS


@pytest.mark.parametrize("bad", sorted(BAD_SPECS))
def test_invalid_spec_is_refused_by_every_entry(product_lib, bad):
    over, what = BAD_SPECS[bad]
    spec = _spec(**over)
    out = C.c_uint64(7)
    assert product_lib.hrt_power_profiles_scratch_bytes(None, None, C.byref(spec), C.byref(out)) == HRT_E_INVALID
    assert out.value == 7
    assert what.encode() in product_lib.hrt_last_error()
    assert product_lib.hrt_power_profiles(None, None, None, C.byref(spec), None, 0, None, 0, None) == HRT_E_INVALID
    assert b"hrt_power_profiles" in product_lib.hrt_last_error()
    # the drop-in entry refuses it before it creates a problem (no device needed to get the answer)
    with pytest.raises(RuntimeError, match=r"hrt_compute_power_profiles failed \(-1\)"):
        abi.run_compute_power_profiles(product_lib, *K.args(K.small(K.C1, 64)), spec)
    assert what.encode() in product_lib.hrt_last_error()


def _endpoints(n):
    return [[float(i), 0.0, 1.0] for i in range(n)]


@pytest.mark.parametrize("nrx,ntx,over,what", [
    (256, 256, {}, "num_rx * num_tx"),
    (64, 64, dict(num_delay_bins=(1 << 14) + 1), "2^26"),
    (8, 8, dict(num_delay_bins=1 << 16, num_zenith_bins=128, num_azimuth_bins=128 * 8), "num_zenith_bins"),
    (32, 32, dict(num_delay_bins=1 << 16, num_zenith_bins=128, num_azimuth_bins=128), "2^26"),
])
def test_link_limits_are_refused_by_the_drop_in(product_lib, nrx, ntx, over, what):
    c = dict(K.small(K.C1, 64))
    c["rx_pos"], c["rx_vel"] = _endpoints(nrx), [[0.0, 0.0, 0.0]] * nrx
    c["tx_pos"], c["tx_vel"] = _endpoints(ntx), [[0.0, 0.0, 0.0]] * ntx
    with pytest.raises(RuntimeError, match=r"hrt_compute_power_profiles failed \(-1\)"):
        abi.run_compute_power_profiles(product_lib, *K.args(c), _spec(**over))
    assert what.encode() in product_lib.hrt_last_error()


def test_largest_spec_passes_the_spec_check(product_lib):
    """Ld = 2^16, Nth * Nph = 2^14, one of each angle and the LoS / scatter parts alone pass the spec check (what
    fails without a problem is the NULL problem)"""
    for over in (dict(num_delay_bins=1 << 16, num_zenith_bins=128, num_azimuth_bins=128),
                 dict(num_delay_bins=0, num_zenith_bins=1, num_azimuth_bins=1 << 14),
                 dict(num_delay_bins=0, tau0=math.nan, dtau=0.0), dict(num_delay_bins=1, tau0=-1.0, dtau=1e-300),
                 dict(parts=abi.CHANNEL_LOS), dict(parts=abi.CHANNEL_SCATTER)):
        spec = _spec(**over)
        assert product_lib.hrt_power_profiles_scratch_bytes(None, None, C.byref(spec), None) == HRT_E_INVALID
        assert b"NULL" in product_lib.hrt_last_error(), over


def _pybind():
    import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    return hermespy_rt


PYBIND_BAD = {
    "delay_bins_over_2_16": (dict(num_delay_bins=(1 << 16) + 1), "num_delay_bins"),
    "tau0_nan": (dict(tau0=math.nan), "tau0"),
    "dtau_zero": (dict(dtau=0.0), "dtau"),
    "zenith_only": (dict(num_zenith_bins=3), "num_azimuth_bins"),
    "angles_over_2_14": (dict(num_zenith_bins=1 << 7, num_azimuth_bins=(1 << 7) + 1), "2\\^14"),
    "no_parts": (dict(los=False, scatter=False), "parts"),
    "bins_over_32_bits": (dict(num_delay_bins=1 << 33), "32 bits"),
}


@pytest.mark.parametrize("bad", sorted(PYBIND_BAD))
def test_pybind_refuses_invalid_spec(bad):
    hermespy_rt = _pybind()
    c = K.small(K.C1, 64)
    args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], 1, 1, 64, 1)
    kw = dict(tau0=0.0, dtau=1e-9, num_delay_bins=64)
    over, what = PYBIND_BAD[bad]
    kw.update(over)
    with pytest.raises(ValueError, match=what):
        hermespy_rt.compute_power_profiles(*args, **kw)


def test_compute_power_profiles_without_device_fails_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny call
    succeeds and returns finite statistics.)"""
    c = K.small(K.C1, 64)
    if _have_gpu():
        d = abi.run_compute_power_profiles(product_lib, *K.args(c), _spec(num_zenith_bins=3, num_azimuth_bins=5))
        assert d["moments"].shape == (1, 1, 2, abi.POWER_FIELDS) and np.isfinite(d["buffer"]).all()
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_power_profiles failed \(-3\)") as e:
        abi.run_compute_power_profiles(product_lib, *K.args(c), _spec())
    assert "HIP" in str(e.value)
