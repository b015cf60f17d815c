"""Argument checks of the equalizer entries (hrt_channel_equalizer, hrt_compute_channel_equalizer,
hermespy_rt.compute_channel_equalizer): a refused call returns HRT_E_INVALID before the device is touched, so these run
without a GPU.  hrt_channel_equalizer has no problem handle that a test could leave out, so a spec is shown to pass a
check by the later check that then refuses the call (a NULL output pointer), never by a launch on made-up pointers.
Without a device a valid call fails loudly (HRT_E_HIP), never with a CPU result."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi

from . import configs as K
from . import equalizer_util as U

HRT_E_INVALID, HRT_E_HIP = -1, -3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000   # a stand-in for a device pointer: tested for NULL only, never read
FIELDS = ["num_rx", "num_tx", "nr", "nt", "num_times", "num_freqs", "kind", "flags", "noise"]


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _el(n):
    return np.arange(3 * n, dtype=np.float32).reshape(n, 3) * 1e-3


def _spec(**over):
    kw = dict(num_rx=2, num_tx=1, nr=4, nt=2, num_times=3, num_freqs=5, noise=0.5, kind=abi.EQ_LMMSE, flags=abi.EQ_W)
    kw.update(over)
    return abi.equalizer_spec(**kw)


def test_equalizer_spec_struct_and_constants_match_c(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hermespy_rt.h"\n'
                    'int main(void){printf("%zu' + ' %zu' * len(FIELDS) + ' %u %u %u %u %u\\n", '
                    "sizeof(hrt_equalizer_spec)" + "".join(", offsetof(hrt_equalizer_spec, %s)" % f for f in FIELDS) +
                    ', HRT_EQ_ZF, HRT_EQ_LMMSE, HRT_EQ_W, HRT_EQ_SINGULAR, HRT_EQ_NONFINITE);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = abi.EqualizerSpec
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + [
        abi.EQ_ZF, abi.EQ_LMMSE, abi.EQ_W, abi.EQ_SINGULAR, abi.EQ_NONFINITE]
    assert (abi.EQ_ZF, abi.EQ_LMMSE, abi.EQ_W, abi.EQ_SINGULAR, abi.EQ_NONFINITE) == (
        U.ZF, U.LMMSE, U.FLAG_W, U.SINGULAR, U.NONFINITE)
    assert abi.equalizer_kind("ZF") == abi.EQ_ZF and abi.equalizer_kind("lmmse") == abi.EQ_LMMSE
    with pytest.raises(ValueError, match="kind"):
        abi.equalizer_kind("mmse")


def test_out_bytes(product_lib):
    for nrx, ntx, nr, nt, T, K_, flags in ((1, 1, 1, 1, 1, 1, 0), (2, 3, 5, 3, 2, 7, 1), (2, 3, 3, 5, 2, 7, 1),
                                           (1, 2, 64, 16, 1, 4, 0), (4, 4, 64, 16, 4, 64, 1)):
        spec = _spec(num_rx=nrx, num_tx=ntx, nr=nr, nt=nt, num_times=T, num_freqs=K_, flags=flags)
        want_bytes = U.out_bytes(nrx, ntx, nr, nt, T, K_, flags)
        assert product_lib.hrt_equalizer_out_bytes(C.byref(spec)) == want_bytes == abi.equalizer_regions(spec)[3]
    assert product_lib.hrt_equalizer_out_bytes(None) == 0
    # an absent region has size 0; the views have the shapes of the header
    o = abi.equalizer_regions(_spec(flags=0))
    assert o[0] == o[1] == 0
    spec = _spec()
    v = abi.equalizer_views(np.zeros(abi.equalizer_regions(spec)[3], np.uint8), spec)
    assert v["W"].shape == (2, 1, 2, 4, 2, 3, 5) and v["W"].dtype == np.complex64
    assert v["sinr"].shape == (2, 1, 2, 2, 3, 5) and v["status"].shape == (2, 1, 2, 3, 5)
    assert abi.equalizer_views(np.zeros(abi.equalizer_regions(_spec(flags=0))[3], np.uint8), _spec(flags=0))["W"] is None


# name -> (spec overrides, what the message names)
BAD_SPEC = {
    "zero_num_rx": (dict(num_rx=0), "must be > 0"),
    "zero_num_tx": (dict(num_tx=0), "must be > 0"),
    "zero_num_times": (dict(num_times=0), "must be > 0"),
    "zero_num_freqs": (dict(num_freqs=0), "must be > 0"),
    "zero_nr": (dict(nr=0), "nr 1 .. 64"),
    "zero_nt": (dict(nt=0), "nt 1 .. 16"),
    "nt_17": (dict(nr=17, nt=17), "nt 1 .. 16"),
    "nt_17_tall": (dict(nr=64, nt=17), "nt 1 .. 16"),
    "nr_65": (dict(nr=65, nt=1), "nr 1 .. 64"),
    "zf_wide": (dict(nr=3, nt=4, kind=abi.EQ_ZF), "nr >= nt"),
    "zf_wide_1": (dict(nr=1, nt=16, kind=abi.EQ_ZF), "nr >= nt"),
    "unknown_kind": (dict(kind=2), "neither"),
    "unknown_kind_all_bits": (dict(kind=0xffffffff), "neither"),
    "flags_unknown_bit": (dict(flags=2), "unknown bits"),
    "flags_all_bits": (dict(flags=0xffffffff), "unknown bits"),
    "noise_zero": (dict(noise=0.0), "noise"),
    "noise_negative": (dict(noise=-1.0), "noise"),
    "noise_nan": (dict(noise=math.nan), "noise"),
    "noise_inf": (dict(noise=math.inf), "noise"),
    "noise_zero_zf": (dict(noise=0.0, kind=abi.EQ_ZF), "noise"),
    "points_over_2_24": (dict(nr=64, nt=16, num_times=128, num_freqs=129), "2^24"),
    "points_wrap_64_bits": (dict(nr=64, nt=16, num_times=0xffffffff, num_freqs=0xffffffff), "2^24"),
    "too_many_points": (dict(num_rx=1 << 16, num_tx=1 << 15, nr=1, nt=1), "2^31 points"),
}

# the largest values that pass: the call is then refused for its NULL output, the check after the spec's
AT_LIMIT = {
    "nt_16": dict(nr=16, nt=16),
    "nr_64": dict(nr=64, nt=16),
    "zf_square": dict(nr=16, nt=16, kind=abi.EQ_ZF),
    "lmmse_wide": dict(nr=1, nt=16),
    "points_2_24": dict(nr=64, nt=16, num_times=128, num_freqs=128),
    "flags_0": dict(flags=0),
    "noise_tiny": dict(noise=1e-38),
    "noise_huge": dict(noise=3e38),
    "all_ones": dict(num_rx=1, num_tx=1, nr=1, nt=1, num_times=1, num_freqs=1),
    "points_below_2_31": dict(num_rx=1 << 15, num_tx=(1 << 15) - 1, nr=1, nt=1, num_times=1, num_freqs=1),
}


@pytest.mark.parametrize("bad", sorted(BAD_SPEC))
def test_device_entry_refuses_the_spec(product_lib, bad):
    over, what = BAD_SPEC[bad]
    spec = _spec(**over)
    assert product_lib.hrt_channel_equalizer(0, C.byref(spec), PTR, PTR, None) == HRT_E_INVALID
    msg = product_lib.hrt_last_error()
    assert b"hrt_channel_equalizer" in msg and what.encode() in msg, msg


@pytest.mark.parametrize("name", sorted(AT_LIMIT))
def test_device_entry_accepts_the_spec_at_its_limits(product_lib, name):
    spec = _spec(**AT_LIMIT[name])
    assert product_lib.hrt_channel_equalizer(0, C.byref(spec), PTR, None, None) == HRT_E_INVALID
    assert b"hrt_channel_equalizer: NULL device pointer" in product_lib.hrt_last_error()


def test_device_entry_refuses_null_pointers(product_lib):
    L, spec = product_lib, _spec()
    assert L.hrt_channel_equalizer(0, None, PTR, PTR, None) == HRT_E_INVALID
    assert b"hrt_channel_equalizer: NULL spec" in L.hrt_last_error()
    for args in ((None, PTR), (PTR, None)):
        assert L.hrt_channel_equalizer(0, C.byref(spec), *args, None) == HRT_E_INVALID
        assert b"hrt_channel_equalizer: NULL device pointer" in L.hrt_last_error()
    with pytest.raises(RuntimeError, match=r"hrt_channel_equalizer failed \(-1\)"):
        abi.run_channel_equalizer(L, 0, spec, PTR, None)


def test_form_rule_of_the_header_refuses_what_the_entry_refuses():
    for nr, nt in ((0, 4), (4, 0), (17, 17), (65, 1), (16, 64)):
        assert U.form(nr, nt) == 0
    for nr, nt in ((1, 1), (16, 16), (64, 16), (1, 16), (64, 1)):
        assert U.form(nr, nt) > 0


# ---------------------------------------------------------------------------------------------- the drop-in entry

def _drop_in(lib, nr=4, nt=2, num_times=1, num_freqs=4, kind=abi.EQ_LMMSE, flags=abi.EQ_W, noise=0.5, parts=None,
             fa=3.5e9, df=1e6, out="array", rx_el=None, nrx=None):
    """hrt_compute_channel_equalizer as called: every argument explicit, nothing derived (a refusal comes before any
    pointer is read, so the counts need not match the arrays) -> (rc, message)"""
    c = K.small(K.C1, 64)
    scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces = K.args(c)
    rx_pos = np.asarray(rx_pos, np.float32).reshape(-1, 3)
    tx_pos = np.asarray(tx_pos, np.float32).reshape(-1, 3)
    rx_vel = np.asarray(rx_vel, np.float32).reshape(-1, 3)
    tx_vel = np.asarray(tx_vel, np.float32).reshape(-1, 3)
    V3 = C.POINTER(abi.Vec3)
    spec = abi.channel_spec(3.5e9, df, num_freqs, 0.0, 0.0, num_times,
                            parts=abi.CHANNEL_LOS | abi.CHANNEL_SCATTER if parts is None else parts)
    re = _el(min(nr, 1025)) if rx_el is None else rx_el
    te = _el(min(nt, 1025))
    oa = np.zeros(1 << 12, np.uint8)
    scene = lib.scene_load(str(scene_path).encode())
    try:
        rc = lib.hrt_compute_channel_equalizer(
            C.byref(scene), rx_pos.ctypes.data_as(V3), tx_pos.ctypes.data_as(V3), rx_vel.ctypes.data_as(V3),
            tx_vel.ctypes.data_as(V3), C.c_float(f_ghz), rx_pos.shape[0] if nrx is None else nrx, tx_pos.shape[0],
            int(num_paths), int(num_bounces), C.byref(spec), re.ctypes.data_as(V3), nr, te.ctypes.data_as(V3), nt,
            C.c_double(fa), kind, flags, C.c_float(noise), oa.ctypes.data_as(C.c_void_p) if out == "array" else None,
            None)
    finally:
        abi.free_scene(scene)
    return rc, lib.hrt_last_error()


_NAN_EL = _el(4)
_NAN_EL[1, 2] = math.nan

# name -> (arguments of _drop_in, what the message names)
BAD_DROP_IN = {
    # hrt_channel_equalizer's refusals
    "nt_17": (dict(nr=17, nt=17), "nt 1 .. 16"),
    "nr_65": (dict(nr=65, nt=2), "nr 1 .. 64"),
    "zf_wide": (dict(nr=2, nt=4, kind=abi.EQ_ZF), "nr >= nt"),
    "unknown_kind": (dict(kind=7), "neither"),
    "flags_unknown_bit": (dict(flags=8), "unknown bits"),
    "noise_zero": (dict(noise=0.0), "noise"),
    "noise_negative": (dict(noise=-2.0), "noise"),
    "noise_nan": (dict(noise=math.nan), "noise"),
    "noise_inf": (dict(noise=math.inf), "noise"),
    "null_out": (dict(out=None), "hrt_compute_channel_equalizer: NULL argument"),
    "zero_num_rx": (dict(nrx=0), "must be > 0"),
    # hrt_compute_array_channel's refusals
    "zero_nr": (dict(nr=0), "0 RX and 2 TX elements"),
    "zero_nt": (dict(nt=0), "4 RX and 0 TX elements"),
    "zero_num_freqs": (dict(num_freqs=0), "num_freqs"),
    "zero_num_times": (dict(num_times=0), "num_times"),
    "points_over_2_24": (dict(nr=64, nt=16, num_times=128, num_freqs=129), "2^24"),
    "no_parts": (dict(parts=0), "parts"),
    "unknown_part": (dict(parts=abi.CHANNEL_LOS | 4), "parts"),
    "fa_zero": (dict(fa=0.0), "array frequency"),
    "fa_inf": (dict(fa=math.inf), "array frequency"),
    "df_nan": (dict(df=math.nan), "finite"),
    "offset_not_finite": (dict(rx_el=_NAN_EL), "RX element 1"),
}


@pytest.mark.parametrize("bad", sorted(BAD_DROP_IN))
def test_drop_in_refuses_invalid_call(product_lib, bad):
    kw, what = BAD_DROP_IN[bad]
    rc, msg = _drop_in(product_lib, **kw)
    assert rc == HRT_E_INVALID, msg
    assert what.encode() in msg, msg


def test_runner_reports_a_refusal(product_lib):
    c = K.small(K.C1, 64)
    spec = abi.channel_spec(3.5e9, 1e6, 4)
    with pytest.raises(RuntimeError, match=r"hrt_compute_channel_equalizer failed \(-1\)"):
        abi.run_compute_channel_equalizer(product_lib, *K.args(c), spec, _el(17), _el(17), 1.0)
    assert b"nt 1 .. 16" in product_lib.hrt_last_error()
    with pytest.raises(RuntimeError, match=r"hrt_compute_channel_equalizer failed \(-1\)"):
        abi.run_compute_channel_equalizer(product_lib, *K.args(c), spec, _el(4), _el(2), 1.0, flags=4)
    assert b"unknown bits" in product_lib.hrt_last_error()
    with pytest.raises(RuntimeError, match=r"hrt_compute_channel_equalizer failed \(-1\)"):
        abi.run_compute_channel_equalizer(product_lib, *K.args(c), spec, _el(2), _el(4), 1.0, kind="zf")
    assert b"nr >= nt" in product_lib.hrt_last_error()
    with pytest.raises(RuntimeError, match=r"hrt_compute_channel_equalizer failed \(-1\)"):
        abi.run_compute_channel_equalizer(product_lib, *K.args(c), spec, _el(4), _el(2), -1.0)
    assert b"noise" in product_lib.hrt_last_error()


# ---------------------------------------------------------------------------------------------- the pybind entry

def _pybind():
    import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    return hermespy_rt


PYBIND_BAD = {
    "nt_17": (dict(rx_elements=_el(17), tx_elements=_el(17)), "nt 1 .. 16"),
    "nr_65": (dict(rx_elements=_el(65)), "nr 1 .. 64"),
    "zf_wide": (dict(rx_elements=_el(2), tx_elements=_el(4), kind="zf"), "nr >= nt"),
    "unknown_kind": (dict(kind="mmse"), "kind must be"),
    "noise_zero": (dict(noise=0.0), "noise"),
    "noise_nan": (dict(noise=math.nan), "noise"),
    "noise_inf": (dict(noise=math.inf), "noise"),
    "zero_nr": (dict(rx_elements=np.zeros((0, 3), np.float32)), "0 RX and 2 TX elements"),
    "zero_num_freqs": (dict(num_freqs=0), "num_freqs"),
    "points_over_2_24": (dict(rx_elements=_el(64), tx_elements=_el(16), num_times=128, num_freqs=129), r"2\^24"),
    "fa_nan": (dict(array_frequency=math.nan), "array frequency"),
    "no_parts": (dict(los=False, scatter=False), "parts"),
    "offset_not_finite": (dict(rx_elements=_NAN_EL), "RX element 1"),
}


@pytest.mark.parametrize("bad", sorted(PYBIND_BAD))
def test_pybind_refuses_invalid_call(bad):
    hermespy_rt = _pybind()
    c = K.small(K.C1, 64)
    args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], 1, 1, 64, 1)
    kw = dict(f0=3.5e9, df=1e6, num_freqs=4, rx_elements=_el(4), tx_elements=_el(2), noise=0.5)
    over, what = PYBIND_BAD[bad]
    kw.update(over)
    with pytest.raises(ValueError, match=what):
        hermespy_rt.compute_channel_equalizer(*args, **kw)


def test_channel_equalizer_without_device_fails_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny call
    succeeds and returns a finite SINR.)"""
    c = K.small(K.C1, 64)
    call = lambda: abi.run_compute_channel_equalizer(product_lib, *K.args(c), abi.channel_spec(3.5e9, 1e6, 4), _el(4),
                                                     _el(2), 1e-12)
    if _have_gpu():
        r = call()
        assert r["sinr"].shape == (1, 1, 2, 2, 1, 4) and np.isfinite(r["sinr"]).all()
        assert r["W"].shape == (1, 1, 2, 4, 2, 1, 4) and r["status"].shape == (1, 1, 2, 1, 4)
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_channel_equalizer failed \(-3\)") as e:
        call()
    assert "HIP" in str(e.value)
