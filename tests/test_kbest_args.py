"""Argument checks of the K-best detection entries (hrt_channel_kbest, hrt_compute_channel_kbest,
hermespy_rt.compute_channel_kbest): a refused call returns HRT_E_INVALID before the device is touched, so these run
without a GPU.  hrt_channel_kbest has no problem handle that a test could leave out, so a spec is shown to pass a
check by the later check that then refuses the call (a NULL output pointer), never by a launch on made-up pointers.
Without a device a valid call fails loudly (HRT_E_HIP), never with a CPU result."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi, detect

from . import configs as K
from . import kbest_util as U

HRT_E_INVALID, HRT_E_HIP = -1, -3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000   # a stand-in for a device pointer: tested for NULL only, never read
FIELDS = ["num_rx", "num_tx", "nr", "nt", "num_times", "num_freqs", "bits", "flags", "k", "noise", "clip"]


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _el(n):
    return np.arange(3 * n, dtype=np.float32).reshape(n, 3) * 1e-3


def _spec(**over):
    kw = dict(num_rx=2, num_tx=1, nr=3, nt=2, num_times=3, num_freqs=5, bits=4, noise=0.5, k=8, clip=20.0,
              flags=abi.KB_LLR | abi.KB_SORTED)
    kw.update(over)
    return abi.kbest_spec(**kw)


def test_kbest_spec_struct_and_constants_match_c(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hermespy_rt.h"\n'
                    'int main(void){printf("%zu' + ' %zu' * len(FIELDS) + ' %u %u %u %u\\n", '
                    "sizeof(hrt_kbest_spec)" + "".join(", offsetof(hrt_kbest_spec, %s)" % f for f in FIELDS) +
                    ', HRT_KB_LLR, HRT_KB_SORTED, HRT_KB_NONFINITE, HRT_KB_DEFICIENT);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = abi.KbestSpec
    consts = [abi.KB_LLR, abi.KB_SORTED, abi.KB_NONFINITE, abi.KB_DEFICIENT]
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + consts
    assert consts == [U.LLR, U.SORTED, U.NONFINITE, U.DEFICIENT]
    assert (detect.NONFINITE, detect.DEFICIENT) == (U.NONFINITE, U.DEFICIENT)
    assert abi.KB_NO_INDEX == U.NO_INDEX == detect.NO_INDEX == 0xFFFFFFFF
    assert (abi.KB_MAX_NR, abi.KB_MAX_NT, abi.KB_MAX_B, abi.KB_MAX_BITS, abi.KB_MAX_K) == \
        (U.MAX_NR, U.MAX_NT, U.MAX_B, U.MAX_BITS, U.MAX_K)
    assert (detect.KB_MAX_NT, detect.KB_MAX_BITS, detect.KB_MAX_K) == (U.MAX_NT, U.MAX_BITS, U.MAX_K)
    for srt in (False, True):
        for llr in (False, True):
            assert _spec(flags=None, llr=llr, sorted=srt).flags == (abi.KB_LLR if llr else 0) | (abi.KB_SORTED if srt else 0)


def test_out_bytes_with_and_without_llrs(product_lib):
    for nrx, ntx, nr, nt, B, T, K_ in ((1, 1, 1, 1, 1, 1, 1), (2, 3, 3, 5, 2, 2, 7), (2, 3, 64, 1, 8, 2, 7),
                                       (1, 2, 16, 16, 2, 1, 4), (4, 4, 4, 4, 8, 4, 64)):
        sizes = []
        for flags in (0, 1, 2, 3):
            spec = _spec(num_rx=nrx, num_tx=ntx, nr=nr, nt=nt, bits=B, num_times=T, num_freqs=K_, flags=flags)
            want = U.out_bytes(nrx, ntx, nt, B, T, K_, flags)
            assert product_lib.hrt_kbest_out_bytes(C.byref(spec)) == want == abi.kbest_regions(spec)[4]
            sizes.append(want)
        assert sizes[0] == nrx * ntx * 2 * T * K_ * 12
        assert sizes[1] - sizes[0] == nrx * ntx * nt * B * 2 * T * K_ * 4 and sizes[2:] == sizes[:2]
    assert product_lib.hrt_kbest_out_bytes(None) == 0
    spec = _spec()
    v = abi.kbest_views(np.zeros(abi.kbest_regions(spec)[4], np.uint8), spec)
    assert v["index"].shape == v["metric"].shape == v["status"].shape == (2, 1, 2, 3, 5)
    assert v["index"].dtype == v["status"].dtype == np.uint32 and v["metric"].dtype == np.float32
    assert v["llr"].shape == (2, 1, 2, 4, 2, 3, 5) and v["llr"].dtype == np.float32
    bare = _spec(flags=abi.KB_SORTED)
    o = abi.kbest_regions(bare)
    assert o[3] == o[4] and abi.kbest_views(np.zeros(o[4], np.uint8), bare)["llr"] is None


# name -> (spec overrides, what the message names)
BAD_SPEC = {
    "zero_num_rx": (dict(num_rx=0), "must be > 0"),
    "zero_num_tx": (dict(num_tx=0), "must be > 0"),
    "zero_num_times": (dict(num_times=0), "must be > 0"),
    "zero_num_freqs": (dict(num_freqs=0), "must be > 0"),
    "zero_nr": (dict(nr=0), "nr = 0 (1 .. 64)"),
    "nr_65": (dict(nr=65), "nr = 65 (1 .. 64)"),
    "zero_bits": (dict(bits=0), "bits = 0 (1 .. 8)"),
    "bits_9": (dict(bits=9, nt=1), "bits = 9 (1 .. 8)"),
    "zero_nt": (dict(nt=0), "nt * bits <= 32"),
    "nt_17": (dict(nt=17, bits=1), "1 <= nt <= 16"),
    "bits_33_in_all": (dict(nt=11, bits=3), "nt * bits <= 32"),
    "bits_40_in_all": (dict(nt=5, bits=8), "nt * bits <= 32"),
    "product_wraps_32_bits": (dict(nt=1 << 30, bits=4), "nt * bits <= 32"),
    "nt_all_bits": (dict(nt=0xffffffff, bits=1), "nt * bits <= 32"),
    "k_zero": (dict(k=0), "k = 0 (1, 2, 4, .. 64)"),
    "k_3": (dict(k=3), "k = 3 (1, 2, 4, .. 64)"),
    "k_48": (dict(k=48), "k = 48"),
    "k_128": (dict(k=128), "k = 128"),
    "k_all_bits": (dict(k=0xffffffff), "k = 4294967295"),
    "k_2_31": (dict(k=1 << 31), "k = 2147483648"),
    "flags_unknown_bit": (dict(flags=4), "unknown bits"),
    "flags_all_bits": (dict(flags=0xffffffff), "unknown bits"),
    "noise_zero": (dict(noise=0.0), "noise"),
    "noise_negative": (dict(noise=-1.0), "noise"),
    "noise_nan": (dict(noise=math.nan), "noise"),
    "noise_inf": (dict(noise=math.inf), "noise"),
    "clip_zero": (dict(clip=0.0), "clip"),
    "clip_negative": (dict(clip=-1.0), "clip"),
    "clip_nan": (dict(clip=math.nan), "clip"),
    "clip_inf": (dict(clip=math.inf), "clip"),
    "grid_over_2_24": (dict(nr=1, nt=1, bits=1, num_times=4097, num_freqs=4096), "2^24"),
    "matrix_grid_over_2_24": (dict(nr=64, nt=4, bits=3, num_times=256, num_freqs=257), "2^24"),
    "too_many_points": (dict(num_rx=1 << 16, num_tx=1 << 15, num_times=1, num_freqs=1), "2^31 points"),
    "points_wrap_64_bits": (dict(num_times=0xffffffff, num_freqs=0xffffffff), "2^24"),
}

# the largest values that pass: the call is then refused for its NULL output, the check after the spec's
AT_LIMIT = {
    "nr_1": dict(nr=1),
    "nr_64": dict(nr=64),
    "nr_below_nt": dict(nr=2, nt=8),
    "bits_1": dict(bits=1),
    "bits_8": dict(bits=8, nt=1),
    "nt_16": dict(nt=16, bits=2),
    "nt_1": dict(nt=1, bits=1),
    "bits_32_in_all": dict(nt=4, bits=8),
    "eight_by_four": dict(nt=8, bits=4),
    "k_1": dict(k=1),
    "k_64": dict(k=64),
    "noise_tiny": dict(noise=1e-38),
    "noise_huge": dict(noise=3e38),
    "clip_tiny": dict(clip=1e-38),
    "clip_huge": dict(clip=3e38),
    "flags_0": dict(flags=0),
    "flags_llr": dict(flags=1),
    "flags_sorted": dict(flags=2),
    "all_ones": dict(num_rx=1, num_tx=1, nr=1, nt=1, num_times=1, num_freqs=1, bits=1, k=1),
    "matrix_grid_at_2_24": dict(nr=64, nt=4, bits=3, num_times=256, num_freqs=256),
    "points_below_2_31": dict(num_rx=1 << 15, num_tx=(1 << 15) - 1, num_times=1, num_freqs=1),
}


@pytest.mark.parametrize("bad", sorted(BAD_SPEC))
def test_device_entry_refuses_the_spec(product_lib, bad):
    over, what = BAD_SPEC[bad]
    spec = _spec(**over)
    assert not abi.kbest_fits(spec)
    assert product_lib.hrt_channel_kbest(0, C.byref(spec), PTR, PTR, PTR, PTR, None) == HRT_E_INVALID
    msg = product_lib.hrt_last_error()
    assert b"hrt_channel_kbest" in msg and what.encode() in msg, msg


@pytest.mark.parametrize("name", sorted(AT_LIMIT))
def test_device_entry_accepts_the_spec_at_its_limits(product_lib, name):
    spec = _spec(**AT_LIMIT[name])
    assert abi.kbest_fits(spec)
    assert U.form(int(spec.nr), int(spec.nt), int(spec.k)) > 0
    assert product_lib.hrt_channel_kbest(0, C.byref(spec), PTR, PTR, PTR, None, None) == HRT_E_INVALID
    assert b"hrt_channel_kbest: NULL device pointer" in product_lib.hrt_last_error()


def test_device_entry_refuses_null_pointers(product_lib):
    L, spec = product_lib, _spec()
    assert L.hrt_channel_kbest(0, None, PTR, PTR, PTR, PTR, None) == HRT_E_INVALID
    assert b"hrt_channel_kbest: NULL spec" in L.hrt_last_error()
    for args in ((None, PTR, PTR, PTR), (PTR, None, PTR, PTR), (PTR, PTR, None, PTR), (PTR, PTR, PTR, None)):
        assert L.hrt_channel_kbest(0, C.byref(spec), *args, None) == HRT_E_INVALID
        assert b"hrt_channel_kbest: NULL device pointer" in L.hrt_last_error()
    with pytest.raises(RuntimeError, match=r"hrt_channel_kbest failed \(-1\)"):
        abi.run_kbest(L, 0, spec, PTR, PTR, PTR, None)


def test_form_rule_of_the_header_refuses_what_the_entry_refuses():
    for nr, nt, k in ((0, 1, 1), (65, 1, 1), (1, 0, 1), (1, 17, 1), (4, 4, 0), (4, 4, 3), (4, 4, 128)):
        assert U.form(nr, nt, k) == 0 and not abi.kbest_fits(_spec(nr=nr, nt=nt, k=k, bits=1))
    for nr, nt, k in ((1, 1, 1), (64, 16, 64), (64, 1, 1), (1, 16, 1), (2, 8, 32)):
        assert U.form(nr, nt, k) > 0 and abi.kbest_fits(_spec(nr=nr, nt=nt, k=k, bits=2))


# ---------------------------------------------------------------------------------------------- the drop-in entry

def _drop_in(lib, nr=2, nt=2, num_times=1, num_freqs=4, bits=2, flags=3, noise=0.5, k=4, clip=8.0, parts=None, fa=3.5e9, df=1e6,
             out="array", Y="array", constellation="array", rx_el=None, nrx=None):
    """hrt_compute_channel_kbest as called: every argument explicit, nothing derived (a refusal comes before any
    pointer is read, so the counts need not match the arrays) -> (rc, message)"""
    c = K.small(K.C1, 64)
    scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces = K.args(c)
    rx_pos = np.asarray(rx_pos, np.float32).reshape(-1, 3)
    tx_pos = np.asarray(tx_pos, np.float32).reshape(-1, 3)
    rx_vel = np.asarray(rx_vel, np.float32).reshape(-1, 3)
    tx_vel = np.asarray(tx_vel, np.float32).reshape(-1, 3)
    V3 = C.POINTER(abi.Vec3)
    fp = C.POINTER(C.c_float)
    spec = abi.channel_spec(3.5e9, df, num_freqs, 0.0, 0.0, num_times,
                            parts=abi.CHANNEL_LOS | abi.CHANNEL_SCATTER if parts is None else parts)
    re = _el(min(nr, 1025)) if rx_el is None else rx_el
    te = _el(min(nt, 1025))
    oa = np.zeros(1 << 12, np.uint8)
    ya = np.zeros(1 << 12, np.float32)
    sa = np.zeros(1 << 12, np.float32)
    scene = lib.scene_load(str(scene_path).encode())
    try:
        rc = lib.hrt_compute_channel_kbest(
            C.byref(scene), rx_pos.ctypes.data_as(V3), tx_pos.ctypes.data_as(V3), rx_vel.ctypes.data_as(V3),
            tx_vel.ctypes.data_as(V3), C.c_float(f_ghz), rx_pos.shape[0] if nrx is None else nrx, tx_pos.shape[0],
            int(num_paths), int(num_bounces), C.byref(spec), re.ctypes.data_as(V3), nr, te.ctypes.data_as(V3), nt,
            C.c_double(fa), ya.ctypes.data_as(fp) if Y == "array" else None,
            sa.ctypes.data_as(fp) if constellation == "array" else None, bits, flags, k, C.c_float(noise),
            C.c_float(clip),
            oa.ctypes.data_as(C.c_void_p) if out == "array" else None, None)
    finally:
        abi.free_scene(scene)
    return rc, lib.hrt_last_error()


_NAN_EL = _el(2)
_NAN_EL[1, 2] = math.nan

# name -> (arguments of _drop_in, what the message names)
BAD_DROP_IN = {
    # hrt_channel_kbest's refusals
    "nr_65": (dict(nr=65), "nr = 65 (1 .. 64)"),
    "zero_bits": (dict(bits=0), "bits = 0 (1 .. 8)"),
    "bits_9": (dict(bits=9, nt=1), "bits = 9 (1 .. 8)"),
    "nt_17": (dict(nt=17, bits=1), "1 <= nt <= 16"),
    "bits_33_in_all": (dict(nt=11, bits=3), "nt * bits <= 32"),
    "k_zero": (dict(k=0), "k = 0"),
    "k_3": (dict(k=3), "k = 3"),
    "k_128": (dict(k=128), "k = 128"),
    "clip_zero": (dict(clip=0.0), "clip"),
    "clip_nan": (dict(clip=math.nan), "clip"),
    "clip_inf": (dict(clip=math.inf), "clip"),
    "flags_unknown_bit": (dict(flags=4), "unknown bits"),
    "noise_zero": (dict(noise=0.0), "noise"),
    "noise_negative": (dict(noise=-2.0), "noise"),
    "noise_nan": (dict(noise=math.nan), "noise"),
    "noise_inf": (dict(noise=math.inf), "noise"),
    "null_out": (dict(out=None), "hrt_compute_channel_kbest: NULL argument"),
    "null_Y": (dict(Y=None), "hrt_compute_channel_kbest: NULL argument"),
    "null_constellation": (dict(constellation=None), "hrt_compute_channel_kbest: NULL argument"),
    "zero_num_rx": (dict(nrx=0), "must be > 0"),
    # hrt_compute_array_channel's refusals
    "zero_nr": (dict(nr=0), "0 RX and 2 TX elements"),
    "zero_nt": (dict(nt=0), "2 RX and 0 TX elements"),
    "zero_num_freqs": (dict(num_freqs=0), "num_freqs"),
    "zero_num_times": (dict(num_times=0), "num_times"),
    "points_over_2_24": (dict(nr=64, nt=4, bits=3, num_times=256, num_freqs=257), "2^24"),
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
    S = detect.qam(2)
    Y = lambda nr: np.zeros((1, 1, nr, 2, 1, 4), np.complex64)
    run = lambda *a, **kw: abi.run_compute_channel_kbest(product_lib, *K.args(c), spec, *a, **kw)
    for args, kw, what in (((_el(65), _el(2), Y(65), S, 1.0, 4, 8.0), {}, b"nr = 65"),
                           ((_el(2), _el(2), Y(2), S, 1.0, 4, 8.0), dict(flags=4), b"unknown bits"),
                           ((_el(2), _el(2), Y(2), S, -1.0, 4, 8.0), {}, b"noise"),
                           ((_el(2), _el(2), Y(2), S, 1.0, 4, 0.0), {}, b"clip"),
                           ((_el(2), _el(2), Y(2), S, 1.0, 5, 8.0), {}, b"k = 5"),
                           ((_el(2), _el(2), Y(2), S, 1.0, 0, 8.0), {}, b"k = 0"),
                           ((_el(2), _el(5), Y(2), detect.qam(7), 1.0, 4, 8.0), {}, b"nt * bits <= 32"),
                           ((_el(2), _el(17), Y(2), detect.qam(1), 1.0, 4, 8.0), {}, b"1 <= nt <= 16"),
                           ((_el(2), _el(1), Y(2), np.ones(512, np.complex64), 1.0, 4, 8.0), {}, b"bits = 9"),
                           ((_el(2), _el(2), None, S, 1.0, 4, 8.0), {}, b"NULL argument"),
                           ((_el(2), _el(2), Y(2), None, 1.0, 4, 8.0), {}, b"NULL argument")):
        with pytest.raises(RuntimeError, match=r"hrt_compute_channel_kbest failed \(-1\)"):
            run(*args, **kw)
        assert what in product_lib.hrt_last_error()
    with pytest.raises(ValueError, match="2\\^B"):
        run(_el(2), _el(2), Y(2), np.ones(3, np.complex64), 1.0, 4, 8.0)
    with pytest.raises(ValueError, match="expected"):
        run(_el(2), _el(2), Y(3), S, 1.0, 4, 8.0)


# ---------------------------------------------------------------------------------------------- the pybind entry

def _pybind():
    import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    return hermespy_rt


def _y(nr=2, T=1, K_=4):
    return np.zeros((1, 1, nr, 2, T, K_), np.complex64)


PYBIND_BAD = {
    "nr_65": (dict(rx_elements=_el(65), Y=_y(65)), "nr = 65"),
    "nt_17": (dict(tx_elements=_el(17), constellation=detect.qam(1)), "1 <= nt <= 16"),
    "bits_40_in_all": (dict(tx_elements=_el(5), constellation=np.ones(256, np.complex64)), r"nt \* bits <= 32"),
    "k_zero": (dict(k=0), "k = 0"),
    "k_6": (dict(k=6), "k = 6"),
    "k_128": (dict(k=128), "k = 128"),
    "clip_zero": (dict(clip=0.0), "clip"),
    "clip_negative": (dict(clip=-3.0), "clip"),
    "clip_nan": (dict(clip=math.nan), "clip"),
    "clip_inf": (dict(clip=math.inf), "clip"),
    "bits_9": (dict(tx_elements=_el(1), constellation=np.ones(512, np.complex64)), "bits = 9"),
    "constellation_of_3": (dict(constellation=np.ones(3, np.complex64)), "constellation must hold"),
    "constellation_of_1": (dict(constellation=np.ones(1, np.complex64)), "constellation must hold"),
    "constellation_2d": (dict(constellation=np.ones((2, 2), np.complex64)), "constellation must be"),
    "Y_of_other_nr": (dict(Y=_y(3)), "Y must be"),
    "Y_of_other_k": (dict(Y=_y(2, 1, 5)), "Y must be"),
    "Y_5d": (dict(Y=_y()[0]), "Y must be"),
    "noise_zero": (dict(noise=0.0), "noise"),
    "noise_nan": (dict(noise=math.nan), "noise"),
    "noise_inf": (dict(noise=math.inf), "noise"),
    "zero_nr": (dict(rx_elements=np.zeros((0, 3), np.float32), Y=_y(0)), "0 RX and 2 TX elements"),
    "zero_num_freqs": (dict(num_freqs=0, Y=_y(2, 1, 0)), "num_freqs"),
    "points_over_2_24": (dict(rx_elements=_el(64), tx_elements=_el(4), constellation=detect.qam(3), num_times=256,
                              num_freqs=257, Y=np.zeros((1, 1, 64, 2, 256, 257), np.complex64)), r"2\^24"),
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
    kw = dict(f0=3.5e9, df=1e6, num_freqs=4, rx_elements=_el(2), tx_elements=_el(2), Y=_y(), constellation=detect.qam(2),
              noise=0.5, k=4, clip=8.0)
    over, what = PYBIND_BAD[bad]
    kw.update(over)
    with pytest.raises(ValueError, match=what):
        hermespy_rt.compute_channel_kbest(*args, **kw)


def test_channel_kbest_without_device_fails_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny call
    succeeds and returns a valid index.)"""
    c = K.small(K.C1, 64)
    call = lambda: abi.run_compute_channel_kbest(product_lib, *K.args(c), abi.channel_spec(3.5e9, 1e6, 4), _el(2),
                                                  _el(2), _y(), detect.qam(2), 1.0, 4, 8.0)
    if _have_gpu():
        r = call()
        assert r["index"].shape == (1, 1, 2, 1, 4) and (r["index"] < 16).all() and (r["status"] != 1).all()
        assert r["llr"].shape == (1, 1, 2, 2, 2, 1, 4)
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_channel_kbest failed \(-3\)") as e:
        call()
    assert "HIP" in str(e.value)
