"""Argument checks of the antenna-pattern entries (hrt_apply_patterns, hrt_compute_set_patterns and the drop-ins that
read it, the `patterns` keyword of the hermespy_rt path-sum functions): a refused call returns HRT_E_INVALID before the
device is touched, so these run without a GPU.  Without a device a valid call fails loudly (HRT_E_HIP), never with a
CPU result.  (A workspace that is too small needs a problem: tests/test_gpu_patterns.py.)"""
import ctypes as C
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from hermespy_rt_amd import abi
from hermespy_rt_amd import patterns as P

from . import configs as K

HRT_E_INVALID, HRT_E_HIP = -1, -3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000   # a stand-in for a device pointer: tested for NULL only, never read


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _offsets(struct):
    return [C.sizeof(struct)] + [getattr(struct, f).offset for f, _ in struct._fields_]


def test_structs_match_c(tmp_path):
    structs = (("hrt_pattern", abi.Pattern), ("hrt_pattern_spec", abi.PatternSpec), ("hrt_patterns_host", abi.PatternsHost))
    lines = []
    for name, S in structs:
        lines.append('printf("%zu' + " %zu" * len(S._fields_) + '\\n", sizeof(' + name + ")" +
                     "".join(", offsetof(%s, %s)" % (name, f) for f, _ in S._fields_) + ");")
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hrt_device.h"\nint main(void){' + "".join(lines) +
                    'printf("%u %u %u %u\\n", HRT_PATTERN_ISOTROPIC, HRT_PATTERN_DIPOLE, HRT_PATTERN_TR38901, '
                    "HRT_PATTERN_TABLE);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)])
    got = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert got[:3] == [_offsets(S) for _, S in structs]
    assert got[3] == [P.ISOTROPIC, P.DIPOLE, P.TR38901, P.TABLE]
    assert C.sizeof(abi.Pattern) == 24 and C.sizeof(abi.PatternSpec) == 64


def test_kernel_contract_struct_compiles_as_c(tmp_path):
    """csrc/hrt_patterns.h is plain C and its _Static_assert (the kernel-argument offsets of hrt_kpatterns) holds"""
    prog = tmp_path / "k.c"
    prog.write_text('#include "hrt_device.h"\n#include "hrt_patterns.h"\n'
                    "int main(void){return sizeof(hrt_kpatterns) == 200 && HRT_PT_MAX_ZENITH == %d && "
                    "HRT_PT_MAX_AZIMUTH == %d && HRT_PT_MAX_GAIN_DB == %d ? 0 : 1;}\n"
                    % (P.MAX_ZENITH, P.MAX_AZIMUTH, int(P.MAX_GAIN_DB)))
    exe = tmp_path / "k"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(REPO, "include"), "-I",
                           os.path.join(REPO, "hermespy-rt_amd", "csrc"), str(prog), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def _pat(kind=P.TR38901, nz=0, na=0, gain_db=0.0, table=None):
    return abi.Pattern(kind, nz, na, gain_db, table)


# name -> (overrides of one side's hrt_pattern, what the message names); the table pointer is tested for NULL only
BAD = {
    "kind_4": (dict(kind=4), "kind = 4"),
    "kind_huge": (dict(kind=0xFFFFFFFF), "kind"),
    "table_null": (dict(kind=P.TABLE, nz=2, na=1), "table"),
    "zenith_1": (dict(kind=P.TABLE, nz=1, na=4, table=PTR), "num_zenith = 1"),
    "zenith_0": (dict(kind=P.TABLE, nz=0, na=4, table=PTR), "num_zenith = 0"),
    "zenith_182": (dict(kind=P.TABLE, nz=182, na=4, table=PTR), "num_zenith = 182"),
    "azimuth_0": (dict(kind=P.TABLE, nz=4, na=0, table=PTR), "num_azimuth = 0"),
    "azimuth_361": (dict(kind=P.TABLE, nz=4, na=361, table=PTR), "num_azimuth = 361"),
    "gain_nan": (dict(gain_db=math.nan), "gain_db"),
    "gain_inf": (dict(gain_db=math.inf), "gain_db"),
    "gain_minus_inf": (dict(kind=P.ISOTROPIC, gain_db=-math.inf), "gain_db"),
    "gain_over_200": (dict(gain_db=200.5), "gain_db"),
    "gain_under_minus_200": (dict(kind=P.DIPOLE, gain_db=-201.0), "gain_db"),
}


def _drop_in(product_lib, host, cfg=None):
    """hrt_compute_channel under hrt_compute_set_patterns(host), cleared afterwards"""
    c = K.small(K.C1, 64) if cfg is None else cfg
    product_lib.hrt_compute_set_patterns(C.byref(host) if host is not None else None)
    try:
        return abi.run_compute_channel(product_lib, *K.args(c), abi.channel_spec(3e9, 1e6, 4))
    finally:
        product_lib.hrt_compute_set_patterns(None)


def _host(rx=None, tx=None, rx_rot=None, tx_rot=None, nrx=0, ntx=0):
    return abi.PatternsHost(rx or _pat(), tx or _pat(P.ISOTROPIC), rx_rot, tx_rot, nrx, ntx)


@pytest.mark.parametrize("side", ["rx", "tx"])
@pytest.mark.parametrize("bad", sorted(BAD))
def test_invalid_pattern_is_refused_by_the_entry_and_the_setter(product_lib, bad, side):
    over, what = BAD[bad]
    spec = abi.PatternSpec(_pat(), _pat(), None, None)
    setattr(spec, side, _pat(**over))
    # the device entry: before the problem, the shard and the workspace are looked at
    assert product_lib.hrt_apply_patterns(None, None, None, 0, C.byref(spec), None) == HRT_E_INVALID
    msg = product_lib.hrt_last_error()
    assert b"hrt_apply_patterns" in msg and what.encode() in msg and (side + " ").encode() in msg
    # the setter accepts anything; the drop-in call that reads it refuses, before it creates a problem.  (A table
    # pointer that passes the NULL test would be read: the size cases have a table of the largest size behind them.)
    keep = np.zeros((182, 361), np.float32)
    p = _pat(**dict(over, table=keep.ctypes.data)) if over.get("table") else _pat(**over)
    with pytest.raises(RuntimeError, match=r"hrt_compute_channel failed \(-1\)"):
        _drop_in(product_lib, _host(**{side: p}))
    msg = product_lib.hrt_last_error()
    assert b"hrt_compute_set_patterns" in msg and what.encode() in msg and (side + " ").encode() in msg


def test_null_arguments_are_refused(product_lib):
    L = product_lib
    spec = abi.PatternSpec(_pat(), _pat(P.DIPOLE), None, None)
    assert L.hrt_apply_patterns(None, None, None, 0, None, None) == HRT_E_INVALID
    assert b"NULL spec" in L.hrt_last_error()
    shard = __import__("hermespy_rt_amd.lib", fromlist=["Shard"]).Shard(64, 0, 1, 0, 1)
    for p, s, ws in ((None, C.byref(shard), PTR), (None, None, PTR), (None, C.byref(shard), None)):
        assert L.hrt_apply_patterns(p, s, ws, 1 << 30, C.byref(spec), None) == HRT_E_INVALID
        assert b"hrt_apply_patterns: NULL argument" in L.hrt_last_error()


def test_host_contents_are_checked_by_the_drop_in(product_lib):
    """what only the host entries can check: table values, rotation counts, finite rotations"""
    eye = np.eye(3, dtype=np.float32).reshape(1, 9).copy()
    for value, name in ((-1e-6, "negative"), (math.nan, "nan"), (math.inf, "inf")):
        t = np.ones((3, 4), np.float32)
        t[2, 1] = value
        for side in ("rx", "tx"):
            with pytest.raises(RuntimeError, match=r"hrt_compute_channel failed \(-1\)"):
                _drop_in(product_lib, _host(**{side: _pat(P.TABLE, 3, 4, 0.0, t.ctypes.data)}))
            assert (side + " table value 9").encode() in product_lib.hrt_last_error(), name
    two = np.concatenate([eye, eye])
    with pytest.raises(RuntimeError, match=r"hrt_compute_channel failed \(-1\)"):
        _drop_in(product_lib, _host(rx_rot=two.ctypes.data, nrx=2))
    assert b"2 rx rotations, but the call has num_rx = 1" in product_lib.hrt_last_error()
    with pytest.raises(RuntimeError, match=r"hrt_compute_channel failed \(-1\)"):
        _drop_in(product_lib, _host(tx_rot=eye.ctypes.data, ntx=0))
    assert b"0 tx rotations, but the call has num_tx = 1" in product_lib.hrt_last_error()
    bad = eye.copy()
    bad[0, 4] = math.nan
    with pytest.raises(RuntimeError, match=r"hrt_compute_channel failed \(-1\)"):
        _drop_in(product_lib, _host(tx_rot=bad.ctypes.data, ntx=1))
    assert b"tx rotation 0 is not finite" in product_lib.hrt_last_error()
    # a count without a rotation array is not looked at
    _valid_or_hip(product_lib, lambda: _drop_in(product_lib, _host(nrx=7, ntx=9)))


def _valid_or_hip(product_lib, call):
    """a call that passes every check: it runs where there is a device, and fails with HRT_E_HIP where there is none"""
    if _have_gpu():
        return call()
    with pytest.raises(RuntimeError, match=r"failed \(-3\)") as e:
        call()
    assert "HIP" in str(e.value)
    return None


def test_every_path_sum_drop_in_reads_the_setting_and_compute_paths_does_not(product_lib):
    L = product_lib
    c = K.small(K.C1, 64)
    el = np.zeros((2, 3), np.float32)
    w = np.ones((1, 2), np.complex64)
    x = np.ones((1, 2, 8), np.complex64)
    calls = {
        "hrt_compute_channel": lambda: abi.run_compute_channel(L, *K.args(c), abi.channel_spec(3e9, 1e6, 4)),
        "hrt_compute_array_channel": lambda: abi.run_compute_array_channel(L, *K.args(c), abi.channel_spec(3e9, 1e6, 4), el, el),
        "hrt_compute_beam_channel": lambda: abi.run_compute_beam_channel(L, *K.args(c), abi.channel_spec(3e9, 1e6, 4), el, el, w, w),
        "hrt_compute_taps": lambda: abi.run_compute_taps(L, *K.args(c), abi.taps_spec(1e8, 8)),
        "hrt_compute_array_taps": lambda: abi.run_compute_array_taps(L, *K.args(c), abi.taps_spec(1e8, 8), el, el),
        "hrt_compute_beam_taps": lambda: abi.run_compute_beam_taps(L, *K.args(c), abi.taps_spec(1e8, 8), el, el, w, w),
        "hrt_compute_power_profiles": lambda: abi.run_compute_power_profiles(L, *K.args(c), abi.power_spec(0.0, 1e-8, 4)),
        "hrt_compute_dominant_paths": lambda: abi.run_compute_dominant_paths(L, *K.args(c), abi.dominant_spec(4)),
        "hrt_compute_array_covariance": lambda: abi.run_compute_array_covariance(L, *K.args(c), abi.covariance_spec(), el, el),
        "hrt_compute_received_signal": lambda: abi.run_compute_received_signal(L, *K.args(c), abi.taps_spec(1e8, 8), el, el, x),
    }
    bad = _host(rx=_pat(kind=9))
    L.hrt_compute_set_patterns(C.byref(bad))
    try:
        for name, call in calls.items():
            with pytest.raises(RuntimeError, match=name + r" failed \(-1\)"):
                call()
            assert b"rx kind = 9" in L.hrt_last_error(), name
        # compute_paths and the path list never see it: they get past the checks (compute_paths itself has no error
        # code to return and ends the process where there is no device: only where there is one)
        _valid_or_hip(L, lambda: abi.run_compute_paths_list(L, *K.args(c)))
        if _have_gpu():
            abi.run_compute_paths(L, *K.args(c))
        # the setting belongs to the thread that made it
        seen = []
        t = threading.Thread(target=lambda: seen.append(_try(calls["hrt_compute_channel"])))
        t.start()
        t.join()
        assert seen and "(-1)" not in seen[0], seen
    finally:
        L.hrt_compute_set_patterns(None)
    # cleared: the same calls pass the checks again
    _valid_or_hip(L, calls["hrt_compute_channel"])


def _try(call):
    try:
        call()
        return "ok"
    except RuntimeError as e:
        return str(e)


def test_compute_patterns_context_sets_and_clears(product_lib):
    c = K.small(K.C1, 64)
    call = lambda: abi.run_compute_channel(product_lib, *K.args(c), abi.channel_spec(3e9, 1e6, 4))   # noqa: E731
    with abi.compute_patterns(product_lib, rx=dict(kind=5, gain_db=0.0, table=None)):
        with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
            call()
    _valid_or_hip(product_lib, call)
    with abi.compute_patterns(product_lib, rx=P.tr38901(), tx=P.table(np.ones((2, 1))),
                              rx_orientation=P.look_at([1, 0, 0])[None], tx_orientation=P.rotation(0.3)[None]):
        _valid_or_hip(product_lib, call)
    with abi.compute_patterns(product_lib, rx_orientation=np.zeros((3, 3, 3), np.float32)):
        with pytest.raises(RuntimeError, match=r"failed \(-1\)"):
            call()
        assert b"3 rx rotations" in product_lib.hrt_last_error()


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


PYBIND_BAD = {
    "not_a_dict": ("tr38901", "patterns must be None or a dict"),
    "unknown_key": (dict(rx=P.dipole(), gain=3), "unknown key 'gain'"),
    "pattern_not_a_dict": (dict(tx=2), r"patterns\['tx'\] must be a pattern dict"),
    "no_kind": (dict(rx=dict(gain_db=0.0)), "needs kind and gain_db"),
    "kind_4": (dict(rx=dict(kind=4, gain_db=0.0)), "rx kind = 4"),
    "table_null": (dict(tx=dict(kind=3, gain_db=0.0, table=None)), "NULL tx table"),
    "table_1d": (dict(tx=dict(kind=3, gain_db=0.0, table=np.ones(4, np.float32))), "shape"),
    "zenith_1": (dict(rx=dict(kind=3, gain_db=0.0, table=np.ones((1, 4), np.float32))), "rx num_zenith = 1"),
    "zenith_182": (dict(rx=dict(kind=3, gain_db=0.0, table=np.ones((182, 4), np.float32))), "rx num_zenith = 182"),
    "azimuth_361": (dict(tx=dict(kind=3, gain_db=0.0, table=np.ones((4, 361), np.float32))), "tx num_azimuth = 361"),
    "table_negative": (dict(tx=dict(kind=3, gain_db=0.0, table=np.full((2, 2), -1.0, np.float32))), "tx table value 0"),
    "table_nan": (dict(rx=dict(kind=3, gain_db=0.0, table=np.full((2, 2), np.nan, np.float32))), "rx table value 0"),
    "gain_nan": (dict(rx=dict(kind=0, gain_db=math.nan)), "rx gain_db"),
    "gain_over_200": (dict(tx=dict(kind=2, gain_db=250.0)), "tx gain_db"),
    "rotation_shape": (dict(rx_orientation=np.zeros((3, 4), np.float32)), "must have shape"),
    "rotation_count": (dict(tx_orientation=np.zeros((2, 3, 3), np.float32)), "2 tx rotations"),
    "rotation_nan": (dict(rx_orientation=np.full((3, 3), np.nan, np.float32)), "rx rotation 0 is not finite"),
}


@pytest.mark.parametrize("bad", sorted(PYBIND_BAD))
def test_pybind_keyword_refuses_invalid_patterns(bad):
    hermespy_rt = _pybind()
    pat, what = PYBIND_BAD[bad]
    with pytest.raises(ValueError, match=what):
        hermespy_rt.compute_channel(*_pybind_args(), 3e9, 1e6, 4, patterns=pat)


def test_pybind_keyword_is_on_every_path_sum_function_and_clears_itself():
    hermespy_rt = _pybind()
    a = _pybind_args()
    el = np.zeros((2, 3), np.float32)
    w = np.ones((1, 2), np.complex64)
    bad = dict(rx=dict(kind=4, gain_db=0.0))
    calls = {
        "compute_channel": lambda **kw: hermespy_rt.compute_channel(*a, 3e9, 1e6, 4, **kw),
        "compute_array_channel": lambda **kw: hermespy_rt.compute_array_channel(*a, 3e9, 1e6, 4, el, el, **kw),
        "compute_beam_channel": lambda **kw: hermespy_rt.compute_beam_channel(*a, 3e9, 1e6, 4, el, el, w, w, **kw),
        "compute_taps": lambda **kw: hermespy_rt.compute_taps(*a, 1e8, 8, **kw),
        "compute_array_taps": lambda **kw: hermespy_rt.compute_array_taps(*a, 1e8, 8, el, el, **kw),
        "compute_beam_taps": lambda **kw: hermespy_rt.compute_beam_taps(*a, 1e8, 8, el, el, w, w, **kw),
        "compute_received_signal": lambda **kw: hermespy_rt.compute_received_signal(
            *a, 1e8, 8, el, el, np.ones((1, 2, 8), np.complex64), **kw),
        "compute_power_profiles": lambda **kw: hermespy_rt.compute_power_profiles(*a, 0.0, 1e-8, 4, **kw),
        "compute_array_covariance": lambda **kw: hermespy_rt.compute_array_covariance(*a, rx_elements=el, **kw),
        "compute_dominant_paths": lambda **kw: hermespy_rt.compute_dominant_paths(*a, 4, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="rx kind = 4"):
            call(patterns=bad)
        # the guard cleared the setting: the same call without the keyword passes the checks
        if _have_gpu():
            call()
        else:
            with pytest.raises(RuntimeError, match=r"failed \(-3\)"):
                call()
    with pytest.raises(TypeError):
        hermespy_rt.compute_paths(*a, patterns=None)


def test_patterns_without_device_fail_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny call
    succeeds and returns a finite channel.)"""
    host = abi.compute_patterns(product_lib, rx=P.tr38901(), tx=P.dipole(), rx_orientation=P.look_at([0, 1, 0])[None])
    call = lambda: _drop_in(product_lib, host.host)   # noqa: E731
    if _have_gpu():
        h = call()
        assert h.shape == (1, 1, 2, 1, 4) and np.isfinite(h.view(np.float32)).all()
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_channel failed \(-3\)") as e:
        call()
    assert "HIP" in str(e.value)
