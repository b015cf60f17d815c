"""Argument checks of the codebook selection entries (hrt_codebook_select, hrt_compute_codebook_select,
hermespy_rt.compute_codebook_select): a refused call returns HRT_E_INVALID before the device is touched, so these run
without a GPU.  hrt_codebook_select has no problem handle that a test could leave out, so a spec is shown to pass a
check by the later check that then refuses the call (a NULL output pointer), never by a launch on made-up pointers.
Without a device a valid call fails loudly (HRT_E_HIP), never with a CPU result."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi, codebook

from . import codebook_util as U
from . import configs as K

HRT_E_INVALID, HRT_E_HIP = -1, -3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000   # a stand-in for a device pointer: tested for NULL only, never read
FIELDS = ["num_rx", "num_tx", "nr", "nt", "num_times", "num_freqs", "layers", "entries", "subband", "metric", "flags",
          "noise"]


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _el(n):
    return np.arange(3 * n, dtype=np.float32).reshape(n, 3) * 1e-3


def _spec(**over):
    kw = dict(num_rx=2, num_tx=1, nr=2, nt=4, num_times=3, num_freqs=5, layers=2, entries=7, metric=abi.CS_CAPACITY,
              noise=0.5, subband=2, flags=abi.CS_TABLE | abi.CS_EFFECTIVE)
    kw.update(over)
    return abi.codebook_spec(**kw)


def test_codebook_spec_struct_and_constants_match_c(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hermespy_rt.h"\n'
                    'int main(void){printf("%zu' + ' %zu' * len(FIELDS) + ' %u %u %u %u %u\\n", '
                    "sizeof(hrt_codebook_spec)" + "".join(", offsetof(hrt_codebook_spec, %s)" % f for f in FIELDS) +
                    ', HRT_CS_POWER, HRT_CS_CAPACITY, HRT_CS_TABLE, HRT_CS_EFFECTIVE, HRT_CS_NONFINITE);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = abi.CodebookSpec
    consts = [abi.CS_POWER, abi.CS_CAPACITY, abi.CS_TABLE, abi.CS_EFFECTIVE, abi.CS_NONFINITE]
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + consts
    assert consts == [U.POWER, U.CAPACITY, U.TABLE, U.EFFECTIVE, U.NONFINITE]
    assert consts[:2] + consts[4:] == [codebook.POWER, codebook.CAPACITY, codebook.NONFINITE]
    assert abi.CS_NO_INDEX == U.NO_INDEX == codebook.NO_INDEX == 0xFFFFFFFF
    assert (abi.CS_MAX_NR, abi.CS_MAX_NT, abi.CS_MAX_L, abi.CS_MAX_C) == (U.MAX_NR, U.MAX_NT, U.MAX_L, U.MAX_C)
    assert [abi.codebook_metric(k) for k in ("POWER", "Capacity")] == [abi.CS_POWER, abi.CS_CAPACITY]
    with pytest.raises(ValueError, match="metric"):
        abi.codebook_metric("sinr")
    # subband None: wideband; noise None: not read under POWER, refused under CAPACITY
    assert _spec(subband=None).subband == 5
    assert abi.codebook_fits(_spec(metric="power", noise=None)) and not abi.codebook_fits(_spec(noise=None))


def test_out_bytes_for_every_flag_combination(product_lib):
    for nrx, ntx, nr, nt, T, K_, L, Cn, S in ((1, 1, 1, 1, 1, 1, 1, 1, 1), (2, 3, 3, 5, 2, 7, 2, 9, 3),
                                              (2, 3, 5, 3, 2, 7, 3, 4096, 7), (1, 2, 16, 64, 1, 4, 4, 65, 1),
                                              (4, 4, 16, 64, 4, 64, 4, 33, 12)):
        sizes = []
        for flags in (0, 1, 2, 3):
            spec = _spec(num_rx=nrx, num_tx=ntx, nr=nr, nt=nt, num_times=T, num_freqs=K_, layers=L, entries=Cn,
                         subband=S, flags=flags)
            want = U.out_bytes(nrx, ntx, nr, T, K_, L, Cn, S, flags)
            assert product_lib.hrt_codebook_out_bytes(C.byref(spec)) == want == abi.codebook_regions(spec)[5]
            sizes.append(want)
        B = (K_ + S - 1) // S
        assert sizes[0] == nrx * ntx * 2 * T * B * 12
        assert sizes[3] - sizes[2] == sizes[1] - sizes[0] == nrx * ntx * Cn * 2 * T * B * 4
        assert sizes[2] - sizes[0] == nrx * ntx * nr * L * 2 * T * K_ * 8
    assert product_lib.hrt_codebook_out_bytes(None) == 0
    # an absent region has size 0 and no view; the views have the shapes of the header
    spec = _spec()
    v = abi.codebook_views(np.zeros(abi.codebook_regions(spec)[5], np.uint8), spec)
    assert v["index"].shape == v["metric"].shape == v["status"].shape == (2, 1, 2, 3, 3)
    assert v["index"].dtype == v["status"].dtype == np.uint32 and v["metric"].dtype == np.float32
    assert v["table"].shape == (2, 1, 7, 2, 3, 3) and v["effective"].shape == (2, 1, 2, 2, 2, 3, 5)
    bare = _spec(flags=0)
    o = abi.codebook_regions(bare)
    assert o[3] == o[4] == o[5]
    v = abi.codebook_views(np.zeros(o[5], np.uint8), bare)
    assert v["table"] is None and v["effective"] is None


# name -> (spec overrides, what the message names)
BAD_SPEC = {
    "zero_num_rx": (dict(num_rx=0), "must be > 0"),
    "zero_num_tx": (dict(num_tx=0), "must be > 0"),
    "zero_num_times": (dict(num_times=0), "must be > 0"),
    "zero_num_freqs": (dict(num_freqs=0), "must be > 0"),
    "zero_nr": (dict(nr=0), "nr 1 .. 16"),
    "zero_nt": (dict(nt=0), "nt 1 .. 64"),
    "nr_17": (dict(nr=17), "nr 1 .. 16"),
    "nt_65": (dict(nt=65), "nt 1 .. 64"),
    "zero_layers": (dict(layers=0), "layers"),
    "layers_5": (dict(layers=5, nt=8), "layers"),
    "layers_above_nt": (dict(layers=3, nt=2), "layers"),
    "zero_entries": (dict(entries=0), "entries"),
    "entries_4097": (dict(entries=4097), "entries"),
    "zero_subband": (dict(subband=0), "subband"),
    "subband_above_k": (dict(subband=6), "subband"),
    "unknown_metric": (dict(metric=2), "neither"),
    "unknown_metric_all_bits": (dict(metric=0xffffffff), "neither"),
    "flags_unknown_bit": (dict(flags=4), "unknown bits"),
    "flags_all_bits": (dict(flags=0xffffffff), "unknown bits"),
    "noise_zero": (dict(noise=0.0), "noise"),
    "noise_negative": (dict(noise=-1.0), "noise"),
    "noise_nan": (dict(noise=math.nan), "noise"),
    "noise_inf": (dict(noise=math.inf), "noise"),
    "too_many_points": (dict(num_rx=1 << 16, num_tx=1 << 15, num_times=1, num_freqs=1, subband=1), "2^31 points"),
    "points_wrap_64_bits": (dict(num_times=0xffffffff, num_freqs=0xffffffff), "2^31 points"),
    "too_many_table_entries": (dict(num_rx=1 << 9, num_tx=1 << 9, num_times=1, num_freqs=1, subband=1, entries=4096),
                               "2^31 table entries"),
}

# the largest values that pass: the call is then refused for its NULL output, the check after the spec's
AT_LIMIT = {
    "nr_16": dict(nr=16),
    "nt_64": dict(nt=64),
    "layers_4": dict(layers=4),
    "layers_1": dict(layers=1),
    "layers_equal_nt": dict(layers=2, nt=2),
    "nt_1": dict(layers=1, nt=1),
    "entries_1": dict(entries=1),
    "entries_4096": dict(entries=4096),
    "subband_1": dict(subband=1),
    "subband_k": dict(subband=5),
    "power": dict(metric=abi.CS_POWER),
    "noise_not_read_by_power_zero": dict(metric=abi.CS_POWER, noise=0.0),
    "noise_not_read_by_power_negative": dict(metric=abi.CS_POWER, noise=-1.0),
    "noise_not_read_by_power_nan": dict(metric=abi.CS_POWER, noise=math.nan),
    "noise_not_read_by_power_inf": dict(metric=abi.CS_POWER, noise=math.inf),
    "noise_tiny": dict(noise=1e-38),
    "noise_huge": dict(noise=3e38),
    "flags_0": dict(flags=0),
    "flags_table": dict(flags=1),
    "flags_effective": dict(flags=2),
    "all_ones": dict(num_rx=1, num_tx=1, nr=1, nt=1, num_times=1, num_freqs=1, layers=1, entries=1, subband=1),
    "points_below_2_31": dict(num_rx=1 << 15, num_tx=(1 << 15) - 1, num_times=1, num_freqs=1, subband=1, entries=1),
    "table_entries_below_2_31": dict(num_rx=1 << 9, num_tx=(1 << 9) - 1, num_times=1, num_freqs=1, subband=1,
                                     entries=4096),
}


@pytest.mark.parametrize("bad", sorted(BAD_SPEC))
def test_device_entry_refuses_the_spec(product_lib, bad):
    over, what = BAD_SPEC[bad]
    spec = _spec(**over)
    assert not abi.codebook_fits(spec)
    assert product_lib.hrt_codebook_select(0, C.byref(spec), PTR, PTR, PTR, None) == HRT_E_INVALID
    msg = product_lib.hrt_last_error()
    assert b"hrt_codebook_select" in msg and what.encode() in msg, msg


@pytest.mark.parametrize("name", sorted(AT_LIMIT))
def test_device_entry_accepts_the_spec_at_its_limits(product_lib, name):
    spec = _spec(**AT_LIMIT[name])
    assert abi.codebook_fits(spec)
    assert product_lib.hrt_codebook_select(0, C.byref(spec), PTR, PTR, None, None) == HRT_E_INVALID
    assert b"hrt_codebook_select: NULL device pointer" in product_lib.hrt_last_error()


def test_device_entry_refuses_null_pointers(product_lib):
    L, spec = product_lib, _spec()
    assert L.hrt_codebook_select(0, None, PTR, PTR, PTR, None) == HRT_E_INVALID
    assert b"hrt_codebook_select: NULL spec" in L.hrt_last_error()
    for args in ((None, PTR, PTR), (PTR, None, PTR), (PTR, PTR, None)):
        assert L.hrt_codebook_select(0, C.byref(spec), *args, None) == HRT_E_INVALID
        assert b"hrt_codebook_select: NULL device pointer" in L.hrt_last_error()
    with pytest.raises(RuntimeError, match=r"hrt_codebook_select failed \(-1\)"):
        abi.run_codebook_select(L, 0, spec, PTR, PTR, None)


def test_tile_rule_of_the_header_refuses_what_the_entry_refuses():
    for nt, l in ((0, 1), (65, 1), (4, 0), (4, 5), (2, 3)):
        assert U.tile(nt, l) == 0
    for nt, l in ((1, 1), (64, 4), (4, 4), (64, 1)):
        assert U.tile(nt, l) > 0


# ---------------------------------------------------------------------------------------------- the drop-in entry

def _drop_in(lib, nr=2, nt=4, num_times=1, num_freqs=4, layers=2, entries=3, subband=2, metric=abi.CS_CAPACITY,
             flags=3, noise=0.5, parts=None, fa=3.5e9, df=1e6, out="array", codebook="array", rx_el=None, nrx=None):
    """hrt_compute_codebook_select as called: every argument explicit, nothing derived (a refusal comes before any
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
    cb = np.zeros(1 << 12, np.float32)
    scene = lib.scene_load(str(scene_path).encode())
    try:
        rc = lib.hrt_compute_codebook_select(
            C.byref(scene), rx_pos.ctypes.data_as(V3), tx_pos.ctypes.data_as(V3), rx_vel.ctypes.data_as(V3),
            tx_vel.ctypes.data_as(V3), C.c_float(f_ghz), rx_pos.shape[0] if nrx is None else nrx, tx_pos.shape[0],
            int(num_paths), int(num_bounces), C.byref(spec), re.ctypes.data_as(V3), nr, te.ctypes.data_as(V3), nt,
            C.c_double(fa), cb.ctypes.data_as(C.POINTER(C.c_float)) if codebook == "array" else None, layers, entries,
            subband, metric, flags, C.c_float(noise), oa.ctypes.data_as(C.c_void_p) if out == "array" else None, None)
    finally:
        abi.free_scene(scene)
    return rc, lib.hrt_last_error()


_NAN_EL = _el(2)
_NAN_EL[1, 2] = math.nan

# name -> (arguments of _drop_in, what the message names)
BAD_DROP_IN = {
    # hrt_codebook_select's refusals
    "nr_17": (dict(nr=17), "nr 1 .. 16"),
    "nt_65": (dict(nt=65), "nt 1 .. 64"),
    "zero_layers": (dict(layers=0), "layers"),
    "layers_5": (dict(layers=5, nt=8), "layers"),
    "layers_above_nt": (dict(layers=3, nt=2), "layers"),
    "zero_entries": (dict(entries=0), "entries"),
    "entries_4097": (dict(entries=4097), "entries"),
    "zero_subband": (dict(subband=0), "subband"),
    "subband_above_k": (dict(subband=5), "subband"),
    "unknown_metric": (dict(metric=7), "neither"),
    "flags_unknown_bit": (dict(flags=8), "unknown bits"),
    "noise_zero": (dict(noise=0.0), "noise"),
    "noise_negative": (dict(noise=-2.0), "noise"),
    "noise_nan": (dict(noise=math.nan), "noise"),
    "noise_inf": (dict(noise=math.inf), "noise"),
    "null_out": (dict(out=None), "hrt_compute_codebook_select: NULL argument"),
    "null_codebook": (dict(codebook=None), "hrt_compute_codebook_select: NULL argument"),
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
    W = np.ones((3, 4, 2), np.complex64)
    run = lambda *a, **kw: abi.run_compute_codebook_select(product_lib, *K.args(c), spec, *a, **kw)
    for args, kw, what in (((_el(17), _el(4), W), dict(noise=1.0), b"nr 1 .. 16"),
                           ((_el(2), _el(4), W), dict(noise=1.0, flags=4), b"unknown bits"),
                           ((_el(2), _el(4), W), dict(noise=-1.0), b"noise"),
                           ((_el(2), _el(4), W), {}, b"noise"),
                           ((_el(2), _el(4), W), dict(noise=1.0, subband=5), b"subband"),
                           ((_el(2), _el(4), np.ones((3, 4, 5), np.complex64)), dict(noise=1.0), b"layers"),
                           ((_el(2), _el(4), None), dict(noise=1.0), b"NULL argument"),
                           ((_el(2), _el(4), W), dict(noise=1.0, metric=5), b"neither")):
        with pytest.raises(RuntimeError, match=r"hrt_compute_codebook_select failed \(-1\)"):
            run(*args, **kw)
        assert what in product_lib.hrt_last_error()
    with pytest.raises(ValueError, match="metric"):
        run(_el(2), _el(4), W, metric="sinr")


# ---------------------------------------------------------------------------------------------- the pybind entry

def _pybind():
    import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    return hermespy_rt


_W = np.ones((3, 4, 2), np.complex64)
PYBIND_BAD = {
    "nr_17": (dict(rx_elements=_el(17)), "nr 1 .. 16"),
    "nt_65": (dict(tx_elements=_el(65), codebook=np.ones((3, 65, 2), np.complex64)), "nt 1 .. 64"),
    "layers_5": (dict(tx_elements=_el(8), codebook=np.ones((3, 8, 5), np.complex64)), "layers"),
    "zero_layers": (dict(codebook=np.ones((3, 4, 0), np.complex64)), "layers"),
    "zero_entries": (dict(codebook=np.ones((0, 4, 2), np.complex64)), "entries"),
    "entries_4097": (dict(codebook=np.ones((4097, 4, 1), np.complex64)), "entries"),
    "codebook_of_other_nt": (dict(codebook=np.ones((3, 5, 2), np.complex64)), "codebook must have shape"),
    "codebook_1d": (dict(codebook=np.ones(4, np.complex64)), "codebook must have shape"),
    "zero_subband": (dict(subband=0), "subband"),
    "subband_above_k": (dict(subband=5), "subband"),
    "unknown_metric": (dict(metric="sinr"), "metric must be"),
    "noise_missing": (dict(noise=None), "noise"),
    "noise_zero": (dict(noise=0.0), "noise"),
    "noise_nan": (dict(noise=math.nan), "noise"),
    "noise_inf": (dict(noise=math.inf), "noise"),
    "zero_nr": (dict(rx_elements=np.zeros((0, 3), np.float32)), "0 RX and 4 TX elements"),
    "zero_num_freqs": (dict(num_freqs=0, subband=None), "num_freqs"),
    "points_over_2_24": (dict(rx_elements=_el(16), tx_elements=_el(64), codebook=np.ones((3, 64, 2), np.complex64),
                              num_times=128, num_freqs=129), r"2\^24"),
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
    kw = dict(f0=3.5e9, df=1e6, num_freqs=4, rx_elements=_el(2), tx_elements=_el(4), codebook=_W, noise=0.5, subband=2)
    over, what = PYBIND_BAD[bad]
    kw.update(over)
    with pytest.raises(ValueError, match=what):
        hermespy_rt.compute_codebook_select(*args, **kw)


def test_codebook_select_without_device_fails_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny call
    succeeds and returns a valid index.)"""
    c = K.small(K.C1, 64)
    call = lambda: abi.run_compute_codebook_select(product_lib, *K.args(c), abi.channel_spec(3.5e9, 1e6, 4), _el(2),
                                                   _el(4), codebook.dft(4), noise=1e-12, table=True, effective=True)
    if _have_gpu():
        r = call()
        assert r["index"].shape == (1, 1, 2, 1, 1) and (r["index"] < 4).all() and not r["status"].any()
        assert r["table"].shape == (1, 1, 4, 2, 1, 1) and r["effective"].shape == (1, 1, 2, 1, 2, 1, 4)
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_codebook_select failed \(-3\)") as e:
        call()
    assert "HIP" in str(e.value)
