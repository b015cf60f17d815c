"""Argument checks of the precoder entries (hrt_channel_precoder, hrt_compute_channel_precoder,
hermespy_rt.compute_channel_precoder): a refused call returns HRT_E_INVALID before the device is touched, so these run
without a GPU.  hrt_channel_precoder has no problem handle that a test could leave out, so a spec is shown to pass a
check by the later check that then refuses the call (a NULL output pointer), never by a launch on made-up pointers.
Without a device a valid call fails loudly (HRT_E_HIP), never with a CPU result."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi, precode

from . import configs as K
from . import precoder_util as U

HRT_E_INVALID, HRT_E_HIP = -1, -3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000   # a stand-in for a device pointer: tested for NULL only, never read
FIELDS = ["num_rx", "num_tx", "nr", "nt", "num_times", "num_freqs", "kind", "norm", "flags", "noise", "power",
          "regularization"]


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _el(n):
    return np.arange(3 * n, dtype=np.float32).reshape(n, 3) * 1e-3


def _spec(**over):
    kw = dict(num_rx=2, num_tx=1, nr=2, nt=4, num_times=3, num_freqs=5, noise=0.5, kind=abi.PC_RZF, power=2.0,
              regularization=0.25, normalize=abi.PC_TOTAL, flags=abi.PC_P)
    kw.update(over)
    return abi.precoder_spec(**kw)


def test_precoder_spec_struct_and_constants_match_c(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hermespy_rt.h"\n'
                    'int main(void){printf("%zu' + ' %zu' * len(FIELDS) + ' %u %u %u %u %u %u %u %u\\n", '
                    "sizeof(hrt_precoder_spec)" + "".join(", offsetof(hrt_precoder_spec, %s)" % f for f in FIELDS) +
                    ', HRT_PC_MRT, HRT_PC_ZF, HRT_PC_RZF, HRT_PC_TOTAL, HRT_PC_STREAM, HRT_PC_P, HRT_PC_SINGULAR, '
                    'HRT_PC_NONFINITE);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = abi.PrecoderSpec
    consts = [abi.PC_MRT, abi.PC_ZF, abi.PC_RZF, abi.PC_TOTAL, abi.PC_STREAM, abi.PC_P, abi.PC_SINGULAR,
              abi.PC_NONFINITE]
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + consts
    assert consts == [U.MRT, U.ZF, U.RZF, U.TOTAL, U.STREAM, U.FLAG_P, U.SINGULAR, U.NONFINITE]
    assert consts == [precode.MRT, precode.ZF, precode.RZF, precode.TOTAL, precode.STREAM, 1, precode.SINGULAR,
                      precode.NONFINITE]
    assert (abi.PC_MAX_NR, abi.PC_MAX_NT) == (U.MAX_NR, U.MAX_NT)
    assert [abi.precoder_kind(k) for k in ("MRT", "zf", "Rzf")] == [abi.PC_MRT, abi.PC_ZF, abi.PC_RZF]
    assert [abi.precoder_norm(k) for k in ("total", "STREAM")] == [abi.PC_TOTAL, abi.PC_STREAM]
    with pytest.raises(ValueError, match="kind"):
        abi.precoder_kind("mmse")
    with pytest.raises(ValueError, match="normalize"):
        abi.precoder_norm("antenna")
    # regularization None: Nr N0 / Ptot under RZF, not read (0) otherwise
    s = _spec(regularization=None, nr=3, noise=0.5, power=4.0)
    assert s.regularization == np.float32(precode.default_regularization(3, 0.5, 4.0)) == 0.375
    assert _spec(regularization=None, kind="zf").regularization == 0 and _spec(kind="mrt", regularization=None).kind == 0


def test_out_bytes(product_lib):
    for nrx, ntx, nr, nt, T, K_, flags in ((1, 1, 1, 1, 1, 1, 0), (2, 3, 3, 5, 2, 7, 1), (2, 3, 5, 3, 2, 7, 1),
                                           (1, 2, 16, 64, 1, 4, 0), (4, 4, 16, 64, 4, 64, 1)):
        spec = _spec(num_rx=nrx, num_tx=ntx, nr=nr, nt=nt, num_times=T, num_freqs=K_, flags=flags)
        want_bytes = U.out_bytes(nrx, ntx, nr, nt, T, K_, flags)
        assert product_lib.hrt_precoder_out_bytes(C.byref(spec)) == want_bytes == abi.precoder_regions(spec)[3]
    assert product_lib.hrt_precoder_out_bytes(None) == 0
    # an absent region has size 0; the views have the shapes of the header
    o = abi.precoder_regions(_spec(flags=0))
    assert o[0] == o[1] == 0
    spec = _spec()
    v = abi.precoder_views(np.zeros(abi.precoder_regions(spec)[3], np.uint8), spec)
    assert v["P"].shape == (2, 1, 4, 2, 2, 3, 5) and v["P"].dtype == np.complex64
    assert v["sinr"].shape == (2, 1, 2, 2, 3, 5) and v["status"].shape == (2, 1, 2, 3, 5)
    assert abi.precoder_views(np.zeros(abi.precoder_regions(_spec(flags=0))[3], np.uint8), _spec(flags=0))["P"] is None


# name -> (spec overrides, what the message names)
BAD_SPEC = {
    "zero_num_rx": (dict(num_rx=0), "must be > 0"),
    "zero_num_tx": (dict(num_tx=0), "must be > 0"),
    "zero_num_times": (dict(num_times=0), "must be > 0"),
    "zero_num_freqs": (dict(num_freqs=0), "must be > 0"),
    "zero_nr": (dict(nr=0), "nr 1 .. 16"),
    "zero_nt": (dict(nt=0), "nt 1 .. 64"),
    "nr_17": (dict(nr=17, nt=17), "nr 1 .. 16"),
    "nr_17_wide": (dict(nr=17, nt=64), "nr 1 .. 16"),
    "nt_65": (dict(nr=1, nt=65), "nt 1 .. 64"),
    "zf_tall": (dict(nr=4, nt=3, kind=abi.PC_ZF), "nr <= nt"),
    "zf_tall_1": (dict(nr=16, nt=1, kind=abi.PC_ZF), "nr <= nt"),
    "unknown_kind": (dict(kind=3), "none of"),
    "unknown_kind_all_bits": (dict(kind=0xffffffff), "none of"),
    "unknown_norm": (dict(normalize=2), "neither"),
    "unknown_norm_all_bits": (dict(normalize=0xffffffff), "neither"),
    "flags_unknown_bit": (dict(flags=2), "unknown bits"),
    "flags_all_bits": (dict(flags=0xffffffff), "unknown bits"),
    "noise_zero": (dict(noise=0.0), "noise"),
    "noise_negative": (dict(noise=-1.0), "noise"),
    "noise_nan": (dict(noise=math.nan), "noise"),
    "noise_inf": (dict(noise=math.inf), "noise"),
    "noise_zero_mrt": (dict(noise=0.0, kind=abi.PC_MRT), "noise"),
    "power_zero": (dict(power=0.0), "power"),
    "power_negative": (dict(power=-1.0), "power"),
    "power_nan": (dict(power=math.nan), "power"),
    "power_inf": (dict(power=math.inf), "power"),
    "power_zero_zf": (dict(power=0.0, kind=abi.PC_ZF), "power"),
    "regularization_zero": (dict(regularization=0.0), "regularization"),
    "regularization_negative": (dict(regularization=-1.0), "regularization"),
    "regularization_nan": (dict(regularization=math.nan), "regularization"),
    "regularization_inf": (dict(regularization=math.inf), "regularization"),
    "points_over_2_24": (dict(nr=16, nt=64, num_times=128, num_freqs=129), "2^24"),
    "points_wrap_64_bits": (dict(nr=16, nt=64, num_times=0xffffffff, num_freqs=0xffffffff), "2^24"),
    "too_many_points": (dict(num_rx=1 << 16, num_tx=1 << 15, nr=1, nt=1), "2^31 points"),
}

# the largest values that pass: the call is then refused for its NULL output, the check after the spec's
AT_LIMIT = {
    "nr_16": dict(nr=16, nt=16),
    "nt_64": dict(nr=16, nt=64),
    "zf_square": dict(nr=16, nt=16, kind=abi.PC_ZF),
    "rzf_tall": dict(nr=16, nt=1),
    "mrt_tall": dict(nr=16, nt=1, kind=abi.PC_MRT),
    "stream": dict(normalize=abi.PC_STREAM),
    "points_2_24": dict(nr=16, nt=64, num_times=128, num_freqs=128),
    "flags_0": dict(flags=0),
    "noise_tiny": dict(noise=1e-38),
    "noise_huge": dict(noise=3e38),
    "power_tiny": dict(power=1e-38),
    "power_huge": dict(power=3e38),
    "regularization_huge": dict(regularization=3e38),
    "regularization_not_read_by_zf": dict(regularization=-1.0, kind=abi.PC_ZF),
    "regularization_not_read_by_mrt": dict(regularization=math.nan, kind=abi.PC_MRT),
    "all_ones": dict(num_rx=1, num_tx=1, nr=1, nt=1, num_times=1, num_freqs=1),
    "points_below_2_31": dict(num_rx=1 << 15, num_tx=(1 << 15) - 1, nr=1, nt=1, num_times=1, num_freqs=1),
}


@pytest.mark.parametrize("bad", sorted(BAD_SPEC))
def test_device_entry_refuses_the_spec(product_lib, bad):
    over, what = BAD_SPEC[bad]
    spec = _spec(**over)
    assert not abi.precoder_fits(spec)
    assert product_lib.hrt_channel_precoder(0, C.byref(spec), PTR, PTR, None) == HRT_E_INVALID
    msg = product_lib.hrt_last_error()
    assert b"hrt_channel_precoder" in msg and what.encode() in msg, msg


@pytest.mark.parametrize("name", sorted(AT_LIMIT))
def test_device_entry_accepts_the_spec_at_its_limits(product_lib, name):
    spec = _spec(**AT_LIMIT[name])
    assert abi.precoder_fits(spec)
    assert product_lib.hrt_channel_precoder(0, C.byref(spec), PTR, None, None) == HRT_E_INVALID
    assert b"hrt_channel_precoder: NULL device pointer" in product_lib.hrt_last_error()


def test_device_entry_refuses_null_pointers(product_lib):
    L, spec = product_lib, _spec()
    assert L.hrt_channel_precoder(0, None, PTR, PTR, None) == HRT_E_INVALID
    assert b"hrt_channel_precoder: NULL spec" in L.hrt_last_error()
    for args in ((None, PTR), (PTR, None)):
        assert L.hrt_channel_precoder(0, C.byref(spec), *args, None) == HRT_E_INVALID
        assert b"hrt_channel_precoder: NULL device pointer" in L.hrt_last_error()
    with pytest.raises(RuntimeError, match=r"hrt_channel_precoder failed \(-1\)"):
        abi.run_channel_precoder(L, 0, spec, PTR, None)


def test_form_rule_of_the_header_refuses_what_the_entry_refuses():
    for nr, nt in ((0, 4), (4, 0), (17, 17), (1, 65), (64, 16)):
        assert U.form(nr, nt) == 0
    for nr, nt in ((1, 1), (16, 16), (16, 64), (16, 1), (1, 64)):
        assert U.form(nr, nt) > 0


# ---------------------------------------------------------------------------------------------- the drop-in entry

def _drop_in(lib, nr=2, nt=4, num_times=1, num_freqs=4, kind=abi.PC_RZF, norm=abi.PC_TOTAL, flags=abi.PC_P, noise=0.5,
             power=1.0, regularization=0.25, parts=None, fa=3.5e9, df=1e6, out="array", rx_el=None, nrx=None):
    """hrt_compute_channel_precoder as called: every argument explicit, nothing derived (a refusal comes before any
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
        rc = lib.hrt_compute_channel_precoder(
            C.byref(scene), rx_pos.ctypes.data_as(V3), tx_pos.ctypes.data_as(V3), rx_vel.ctypes.data_as(V3),
            tx_vel.ctypes.data_as(V3), C.c_float(f_ghz), rx_pos.shape[0] if nrx is None else nrx, tx_pos.shape[0],
            int(num_paths), int(num_bounces), C.byref(spec), re.ctypes.data_as(V3), nr, te.ctypes.data_as(V3), nt,
            C.c_double(fa), kind, norm, flags, C.c_float(noise), C.c_float(power), C.c_float(regularization),
            oa.ctypes.data_as(C.c_void_p) if out == "array" else None, None)
    finally:
        abi.free_scene(scene)
    return rc, lib.hrt_last_error()


_NAN_EL = _el(2)
_NAN_EL[1, 2] = math.nan

# name -> (arguments of _drop_in, what the message names)
BAD_DROP_IN = {
    # hrt_channel_precoder's refusals
    "nr_17": (dict(nr=17, nt=17), "nr 1 .. 16"),
    "nt_65": (dict(nr=2, nt=65), "nt 1 .. 64"),
    "zf_tall": (dict(nr=4, nt=2, kind=abi.PC_ZF), "nr <= nt"),
    "unknown_kind": (dict(kind=7), "none of"),
    "unknown_norm": (dict(norm=7), "neither"),
    "flags_unknown_bit": (dict(flags=8), "unknown bits"),
    "noise_zero": (dict(noise=0.0), "noise"),
    "noise_negative": (dict(noise=-2.0), "noise"),
    "noise_nan": (dict(noise=math.nan), "noise"),
    "noise_inf": (dict(noise=math.inf), "noise"),
    "power_zero": (dict(power=0.0), "power"),
    "power_nan": (dict(power=math.nan), "power"),
    "power_inf": (dict(power=math.inf), "power"),
    "regularization_zero": (dict(regularization=0.0), "regularization"),
    "regularization_nan": (dict(regularization=math.nan), "regularization"),
    "regularization_inf": (dict(regularization=math.inf), "regularization"),
    "null_out": (dict(out=None), "hrt_compute_channel_precoder: NULL argument"),
    "zero_num_rx": (dict(nrx=0), "must be > 0"),
    # hrt_compute_array_channel's refusals
    "zero_nr": (dict(nr=0), "0 RX and 4 TX elements"),
    "zero_nt": (dict(nt=0), "2 RX and 0 TX elements"),
    "zero_num_freqs": (dict(num_freqs=0), "num_freqs"),
    "zero_num_times": (dict(num_times=0), "num_times"),
    "points_over_2_24": (dict(nr=16, nt=64, num_times=128, num_freqs=129), "2^24"),
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
    run = lambda *a, **kw: abi.run_compute_channel_precoder(product_lib, *K.args(c), spec, *a, **kw)
    for args, kw, what in (((_el(17), _el(17), 1.0), {}, b"nr 1 .. 16"),
                           ((_el(2), _el(4), 1.0), dict(flags=4), b"unknown bits"),
                           ((_el(4), _el(2), 1.0), dict(kind="zf"), b"nr <= nt"),
                           ((_el(2), _el(4), -1.0), {}, b"noise"),
                           ((_el(2), _el(4), 1.0), dict(power=0.0), b"power"),
                           ((_el(2), _el(4), 1.0), dict(regularization=-1.0), b"regularization"),
                           ((_el(2), _el(4), 1.0), dict(normalize=5), b"neither")):
        with pytest.raises(RuntimeError, match=r"hrt_compute_channel_precoder failed \(-1\)"):
            run(*args, **kw)
        assert what in product_lib.hrt_last_error()
    with pytest.raises(ValueError, match="normalize"):
        run(_el(2), _el(4), 1.0, normalize="antenna")


# ---------------------------------------------------------------------------------------------- the pybind entry

def _pybind():
    import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    return hermespy_rt


PYBIND_BAD = {
    "nr_17": (dict(rx_elements=_el(17), tx_elements=_el(17)), "nr 1 .. 16"),
    "nt_65": (dict(tx_elements=_el(65)), "nt 1 .. 64"),
    "zf_tall": (dict(rx_elements=_el(4), tx_elements=_el(2), kind="zf"), "nr <= nt"),
    "unknown_kind": (dict(kind="mmse"), "kind must be"),
    "unknown_norm": (dict(normalize="antenna"), "normalize must be"),
    "noise_zero": (dict(noise=0.0), "noise"),
    "noise_nan": (dict(noise=math.nan), "noise"),
    "noise_inf": (dict(noise=math.inf), "noise"),
    "power_zero": (dict(power=0.0), "power"),
    "power_nan": (dict(power=math.nan), "power"),
    "power_inf": (dict(power=math.inf), "power"),
    "regularization_zero": (dict(regularization=0.0), "regularization"),
    "regularization_nan": (dict(regularization=math.nan), "regularization"),
    "regularization_inf": (dict(regularization=math.inf), "regularization"),
    "zero_nr": (dict(rx_elements=np.zeros((0, 3), np.float32)), "0 RX and 4 TX elements"),
    "zero_num_freqs": (dict(num_freqs=0), "num_freqs"),
    "points_over_2_24": (dict(rx_elements=_el(16), tx_elements=_el(64), num_times=128, num_freqs=129), r"2\^24"),
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
    kw = dict(f0=3.5e9, df=1e6, num_freqs=4, rx_elements=_el(2), tx_elements=_el(4), noise=0.5)
    over, what = PYBIND_BAD[bad]
    kw.update(over)
    with pytest.raises(ValueError, match=what):
        hermespy_rt.compute_channel_precoder(*args, **kw)


def test_channel_precoder_without_device_fails_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny call
    succeeds and returns a finite SINR.)"""
    c = K.small(K.C1, 64)
    call = lambda: abi.run_compute_channel_precoder(product_lib, *K.args(c), abi.channel_spec(3.5e9, 1e6, 4), _el(2),
                                                    _el(4), 1e-12)
    if _have_gpu():
        r = call()
        assert r["sinr"].shape == (1, 1, 2, 2, 1, 4) and np.isfinite(r["sinr"]).all()
        assert r["P"].shape == (1, 1, 4, 2, 2, 1, 4) and r["status"].shape == (1, 1, 2, 1, 4)
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_channel_precoder failed \(-3\)") as e:
        call()
    assert "HIP" in str(e.value)
