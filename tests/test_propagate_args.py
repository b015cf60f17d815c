"""Argument checks of the received-signal entries (hrt_propagate, hrt_compute_received_signal,
hermespy_rt.compute_received_signal): a refused call returns HRT_E_INVALID before the device is touched, so these run
without a GPU.  hrt_propagate has no problem handle that a test could leave out, so a spec is shown to pass a check by
the later check that then refuses the call (accumulate = 2), never by a launch on made-up pointers.  Without a device
a valid call fails loudly (HRT_E_HIP), never with a CPU result."""
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
PTR = 0x1000   # a stand-in for a device pointer: tested for NULL only, never read
FIELDS = ["num_rx", "num_tx", "nr", "nt", "num_times", "num_taps", "l_min", "samples_per_block", "num_samples",
          "num_out"]
COUNTS = [f for f in FIELDS if f != "l_min"]


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _el(n):
    return np.arange(3 * n, dtype=np.float32).reshape(n, 3) * 1e-3


def _spec(**over):
    kw = dict(num_rx=2, num_tx=1, nr=2, nt=2, num_times=1, num_taps=4, l_min=0, samples_per_block=1, num_samples=8,
              num_out=11)
    kw.update(over)
    return abi.propagate_spec(**kw)


def test_propagate_spec_struct_matches_c(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hermespy_rt.h"\n'
                    'int main(void){printf("%zu' + ' %zu' * len(FIELDS) + '\\n", sizeof(hrt_propagate_spec)' +
                    "".join(", offsetof(hrt_propagate_spec, %s)" % f for f in FIELDS) + ');return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = abi.PropagateSpec
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in FIELDS]


def test_out_floats(product_lib):
    for nrx, nr, n_out in ((1, 1, 1), (3, 5, 77), (2, 1024, 1 << 31)):
        spec = _spec(num_rx=nrx, nr=nr, num_out=n_out)
        assert product_lib.hrt_propagate_out_floats(C.byref(spec)) == nrx * nr * 2 * n_out * 2
    assert product_lib.hrt_propagate_out_floats(None) == 0


# name -> (spec overrides, what the message names)
BAD_SPEC = dict({"zero_" + f: ({f: 0}, "must be > 0") for f in COUNTS}, **{
    "nr_over_1024": (dict(nr=1025), "1 .. 1024"),
    "nt_over_1024": (dict(nt=1025), "1 .. 1024"),
    "points_over_2_24": (dict(nr=64, nt=64, num_times=64, num_taps=65), "2^24"),
    "points_wrap_64_bits": (dict(nr=1024, nt=1024, num_times=0xffffffff, num_taps=0xffffffff), "2^24"),
    "l_min_below": (dict(l_min=-(1 << 24) - 1), "tap indices"),
    "l_min_above": (dict(l_min=(1 << 24) + 1), "tap indices"),
    "last_tap_above": (dict(l_min=(1 << 24) - 3, num_taps=4), "tap indices"),
    "num_samples_over_2_31": (dict(num_samples=(1 << 31) + 1), "2^31"),
    "num_out_over_2_31": (dict(num_out=(1 << 31) + 1), "2^31"),
})

# the largest values that pass: the call is then refused for its accumulate = 2, the check after the spec's
AT_LIMIT = {
    "elements_1024": dict(nr=1024, nt=1024, num_times=1, num_taps=16),
    "points_2_24": dict(nr=64, nt=64, num_times=64, num_taps=64),
    "l_min_lowest": dict(l_min=-(1 << 24)),
    "last_tap_2_24": dict(l_min=(1 << 24) - 4, num_taps=4),
    "samples_2_31": dict(num_samples=1 << 31, num_out=1 << 31),
    "all_ones": dict(num_rx=1, num_tx=1, nr=1, nt=1, num_times=1, num_taps=1, samples_per_block=1, num_samples=1,
                     num_out=1),
}


@pytest.mark.parametrize("bad", sorted(BAD_SPEC))
def test_device_entry_refuses_the_spec(product_lib, bad):
    over, what = BAD_SPEC[bad]
    spec = _spec(**over)
    assert product_lib.hrt_propagate(0, C.byref(spec), PTR, PTR, PTR, 0, None) == HRT_E_INVALID
    msg = product_lib.hrt_last_error()
    assert b"hrt_propagate" in msg and what.encode() in msg


@pytest.mark.parametrize("name", sorted(AT_LIMIT))
def test_device_entry_accepts_the_spec_at_its_limits(product_lib, name):
    spec = _spec(**AT_LIMIT[name])
    assert product_lib.hrt_propagate(0, C.byref(spec), PTR, PTR, PTR, 2, None) == HRT_E_INVALID
    assert b"accumulate = 2" in product_lib.hrt_last_error()


def test_device_entry_refuses_null_pointers_and_accumulate(product_lib):
    L, spec = product_lib, _spec()
    assert L.hrt_propagate(0, None, PTR, PTR, PTR, 0, None) == HRT_E_INVALID
    assert b"hrt_propagate: NULL spec" in L.hrt_last_error()
    for args in ((None, PTR, PTR), (PTR, None, PTR), (PTR, PTR, None)):
        assert L.hrt_propagate(0, C.byref(spec), *args, 0, None) == HRT_E_INVALID
        assert b"hrt_propagate: NULL device pointer" in L.hrt_last_error()
    for acc in (2, -1, 256):
        assert L.hrt_propagate(0, C.byref(spec), PTR, PTR, PTR, acc, None) == HRT_E_INVALID
        assert ("accumulate = %d" % acc).encode() in L.hrt_last_error()
    with pytest.raises(RuntimeError, match=r"hrt_propagate failed \(-1\)"):
        abi.run_propagate(L, 0, spec, PTR, PTR, PTR, accumulate=2)


# ---------------------------------------------------------------------------------------------- the drop-in entry

def _drop_in(lib, num_taps=4, num_times=1, l_min=0, s=11, nr=2, nt=2, n=8, num_out=11, fs=1e6, parts=None, fa=3.5e9,
             x="array", y="array", rx_el=None, nrx=None):
    """hrt_compute_received_signal as called: every argument explicit, nothing derived (a refusal comes before any
    pointer is read, so the counts need not match the arrays) -> (rc, message)"""
    c = K.small(K.C1, 64)
    scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces = K.args(c)
    rx_pos = np.asarray(rx_pos, np.float32).reshape(-1, 3)
    tx_pos = np.asarray(tx_pos, np.float32).reshape(-1, 3)
    rx_vel = np.asarray(rx_vel, np.float32).reshape(-1, 3)
    tx_vel = np.asarray(tx_vel, np.float32).reshape(-1, 3)
    V3 = C.POINTER(abi.Vec3)
    spec = abi.taps_spec(fs, num_taps, l_min, 0.0, 0.0, 0.0, num_times,
                         parts=abi.CHANNEL_LOS | abi.CHANNEL_SCATTER if parts is None else parts)
    re = _el(min(nr, 1025)) if rx_el is None else rx_el
    te = _el(min(nt, 1025))
    xa = np.zeros((1, max(min(nt, 4), 1), max(min(n, 64), 1)), np.complex64)
    ya = np.zeros(1 << 12, np.float32)
    scene = lib.scene_load(str(scene_path).encode())
    try:
        rc = lib.hrt_compute_received_signal(
            C.byref(scene), rx_pos.ctypes.data_as(V3), tx_pos.ctypes.data_as(V3), rx_vel.ctypes.data_as(V3),
            tx_vel.ctypes.data_as(V3), C.c_float(f_ghz), rx_pos.shape[0] if nrx is None else nrx, tx_pos.shape[0],
            int(num_paths), int(num_bounces), C.byref(spec), re.ctypes.data_as(V3), nr, te.ctypes.data_as(V3), nt,
            C.c_double(fa), s, xa.ctypes.data_as(abi.c_float_p) if x == "array" else None, n, num_out,
            ya.ctypes.data_as(abi.c_float_p) if y == "array" else None, None)
    finally:
        abi.free_scene(scene)
    return rc, lib.hrt_last_error()


_NAN_EL = _el(2)
_NAN_EL[1, 2] = math.nan

# name -> (arguments of _drop_in, what the message names)
BAD_DROP_IN = {
    # hrt_propagate's refusals
    "zero_num_taps": (dict(num_taps=0), "num_taps and num_times"),
    "zero_num_times": (dict(num_times=0), "num_taps and num_times"),
    "zero_nr": (dict(nr=0), "0 RX and 2 TX elements"),
    "zero_nt": (dict(nt=0), "2 RX and 0 TX elements"),
    "zero_num_rx": (dict(nrx=0), "must be > 0"),
    "zero_samples_per_block": (dict(s=0), "must be > 0"),
    "zero_num_samples": (dict(n=0), "must be > 0"),
    "zero_num_out": (dict(num_out=0), "must be > 0"),
    "nr_over_1024": (dict(nr=1025), "1 .. 1024"),
    "nt_over_1024": (dict(nt=1025), "1 .. 1024"),
    "points_over_2_24": (dict(nr=64, nt=64, num_times=64, num_taps=65), "2^24"),
    "l_min_above": (dict(l_min=(1 << 24) + 1), "tap indices"),
    "l_min_below": (dict(l_min=-(1 << 24) - 1), "tap indices"),
    "last_tap_above": (dict(l_min=(1 << 24) - 3), "tap indices"),
    "num_samples_over_2_31": (dict(n=(1 << 31) + 1), "2^31"),
    "num_out_over_2_31": (dict(num_out=(1 << 31) + 1, s=(1 << 31) + 1), "2^31"),
    "null_x": (dict(x=None), "hrt_compute_received_signal: NULL argument"),
    "null_y": (dict(y=None), "hrt_compute_received_signal: NULL argument"),
    # its own
    "times_not_the_blocks": (dict(num_times=2, s=16, num_out=16), "ceil(num_out / samples_per_block) = 1"),
    "times_short_of_the_blocks": (dict(num_times=1, s=5, num_out=11), "ceil(num_out / samples_per_block) = 3"),
    # hrt_compute_array_taps' refusals
    "fs_zero": (dict(fs=0.0), "sampling rate"),
    "fs_nan": (dict(fs=math.nan), "sampling rate"),
    "no_parts": (dict(parts=0), "parts"),
    "unknown_part": (dict(parts=abi.CHANNEL_LOS | 4), "parts"),
    "taps_times_over_2_20": (dict(num_taps=1 << 11, num_times=(1 << 9) + 1, nr=1, nt=1), "2^20"),
    "fa_zero": (dict(fa=0.0), "array frequency"),
    "fa_inf": (dict(fa=math.inf), "array frequency"),
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
    spec = abi.taps_spec(1e6, 4, num_times=2)
    x = np.zeros((1, 2, 8), np.complex64)
    with pytest.raises(RuntimeError, match=r"hrt_compute_received_signal failed \(-1\)"):
        abi.run_compute_received_signal(product_lib, *K.args(c), spec, _el(2), _el(2), x, samples_per_block=16)
    assert b"ceil" in product_lib.hrt_last_error()
    with pytest.raises(RuntimeError, match=r"hrt_compute_received_signal failed \(-1\)"):
        abi.run_compute_received_signal(product_lib, *K.args(c), abi.taps_spec(1e6, 4), _el(2), _el(2), None)
    assert b"NULL argument" in product_lib.hrt_last_error()


# ---------------------------------------------------------------------------------------------- the pybind entry

def _pybind():
    import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    return hermespy_rt


_X = np.zeros((1, 2, 8), np.complex64)

PYBIND_BAD = {
    "zero_num_taps": (dict(num_taps=0), "num_taps and num_times"),
    "zero_nr": (dict(rx_elements=np.zeros((0, 3), np.float32)), "0 RX and 2 TX elements"),
    "zero_samples_per_block": (dict(samples_per_block=0), "must be > 0"),
    "zero_num_samples": (dict(signal=np.zeros((1, 2, 0), np.complex64)), "must be > 0"),
    "zero_num_out": (dict(num_out=0), "must be > 0"),
    "nr_over_1024": (dict(rx_elements=np.zeros((1025, 3), np.float32)), "1 .. 1024"),
    "points_over_2_24": (dict(rx_elements=np.zeros((1024, 3), np.float32), num_taps=(1 << 13) + 1,
                              samples_per_block=None), r"2\^24"),
    "l_min_above": (dict(l_min=(1 << 24) + 1), "tap indices"),
    "num_out_over_2_31": (dict(num_out=(1 << 31) + 1), r"2\^31"),
    "fs_zero": (dict(sampling_rate=0.0), "sampling rate"),
    "fa_nan": (dict(array_frequency=math.nan), "array frequency"),
    "no_parts": (dict(los=False, scatter=False), "parts"),
    "offset_not_finite": (dict(rx_elements=_NAN_EL), "RX element 1"),
    "ports_differ": (dict(signal=np.zeros((1, 3, 8), np.complex64)), "TX ports"),
    "signal_1d": (dict(signal=np.zeros(8, np.complex64)), "signal must have shape"),
}


@pytest.mark.parametrize("bad", sorted(PYBIND_BAD))
def test_pybind_refuses_invalid_call(bad):
    hermespy_rt = _pybind()
    c = K.small(K.C1, 64)
    args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], 1, 1, 64, 1)
    kw = dict(sampling_rate=1e6, num_taps=4, rx_elements=_el(2), tx_elements=_el(2), signal=_X)
    over, what = PYBIND_BAD[bad]
    kw.update(over)
    with pytest.raises(ValueError, match=what):
        hermespy_rt.compute_received_signal(*args, **kw)


def test_received_signal_without_device_fails_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny call
    succeeds and returns a finite signal.)"""
    c = K.small(K.C1, 64)
    x = (np.arange(16) + 1j).astype(np.complex64).reshape(1, 2, 8)
    call = lambda: abi.run_compute_received_signal(product_lib, *K.args(c), abi.taps_spec(1e6, 4), _el(2), _el(2), x)
    if _have_gpu():
        y = call()
        assert y.shape == (1, 2, 2, 11) and np.isfinite(y.view(np.float32)).all()
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_received_signal failed \(-3\)") as e:
        call()
    assert "HIP" in str(e.value)
