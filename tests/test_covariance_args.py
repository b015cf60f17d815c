"""Argument checks of the covariance entries (hrt_array_covariance_scratch_bytes, hrt_array_covariance,
hrt_compute_array_covariance, hermespy_rt.compute_array_covariance): a refused call returns HRT_E_INVALID before the
device is touched, so these run without a GPU.  Without a device a valid call fails loudly (HRT_E_HIP), never with a
CPU result.  (A scratch that is too small needs a problem: tests/test_gpu_covariance.py.)"""
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
BOTH = abi.COV_RX | abi.COV_TX
PARTS = abi.CHANNEL_LOS | abi.CHANNEL_SCATTER
PTR = 0x1000   # a stand-in for a device pointer: tested for NULL only, never read


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _el(n):
    return np.arange(3 * n, dtype=np.float32).reshape(n, 3) * 1e-3


# name -> (spec overrides, array overrides (nr, nt, rx pointer, tx pointer, f_a), what the message names)
BAD = {
    "no_parts": (dict(parts=0), {}, "parts"),
    "unknown_part": (dict(parts=abi.CHANNEL_SCATTER | 4), {}, "parts"),
    "no_sides": (dict(sides=0), {}, "sides"),
    "unknown_side": (dict(sides=abi.COV_RX | 4), {}, "sides"),
    "rx_zero_elements": ({}, dict(nr=0), "num_rx_elements"),
    "tx_zero_elements": ({}, dict(nt=0), "num_tx_elements"),
    "rx_over_256": ({}, dict(nr=257), "num_rx_elements"),
    "tx_over_256": ({}, dict(nt=257), "num_tx_elements"),
    "tx_over_256_alone": (dict(sides=abi.COV_TX), dict(nr=0, rx=None, nt=1000), "num_tx_elements"),
    "rx_null_elements": ({}, dict(rx=None), "rx_elements"),
    "tx_null_elements": ({}, dict(tx=None), "tx_elements"),
    "fa_nan": ({}, dict(fa=math.nan), "array frequency"),
    "fa_inf": ({}, dict(fa=math.inf), "array frequency"),
    "fa_zero": ({}, dict(fa=0.0), "array frequency"),
    "fa_negative": ({}, dict(fa=-1e9), "array frequency"),
}


def _spec(parts=PARTS, sides=BOTH):
    return abi.covariance_spec(parts=parts, sides=sides)


def _arrays(nr=4, nt=3, rx=PTR, tx=PTR, fa=3.5e9):
    return abi.ArraySpec(nr, nt, rx, tx, fa)


def test_covariance_spec_struct_matches_c(tmp_path):
    fields = ["parts", "sides"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hrt_device.h"\n'
                    'int main(void){printf("%zu' + ' %zu' * len(fields) + ' %u %u\\n", sizeof(hrt_covariance_spec)' +
                    "".join(", offsetof(hrt_covariance_spec, %s)" % f for f in fields) +
                    ', HRT_COV_RX, HRT_COV_TX);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S = abi.CovarianceSpec
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields] + [abi.COV_RX, abi.COV_TX]


def test_kernel_contract_struct_compiles_as_c(tmp_path):
    """csrc/hrt_covariance.h is plain C and its _Static_asserts (the kernel-argument offsets of hrt_kcov) hold"""
    prog = tmp_path / "k.c"
    prog.write_text('#include "hrt_device.h"\n#include "hrt_covariance.h"\n'
                    'int main(void){return sizeof(hrt_kcov) == 192 && HRT_CV_MAX_ELEMENTS == %d ? 0 : 1;}\n'
                    % abi.COV_MAX_ELEMENTS)
    exe = tmp_path / "k"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(REPO, "include"), "-I",
                           os.path.join(REPO, "hermespy-rt_amd", "csrc"), str(prog), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def test_out_floats(product_lib):
    for nrx, ntx, nr, nt, sides in ((1, 1, 1, 1, BOTH), (3, 5, 7, 2, BOTH), (2, 2, 16, 9, abi.COV_RX),
                                    (2, 2, 16, 9, abi.COV_TX), (4, 1, 256, 256, BOTH)):
        spec, a = _spec(sides=sides), _arrays(nr, nt)
        want = abi.covariance_out_floats(nrx, ntx, a, spec)
        assert product_lib.hrt_covariance_out_floats(nrx, ntx, C.byref(a), C.byref(spec)) == want
        assert want == abi.covariance_out_floats(nrx, ntx, (nr, nt), spec)
        assert want == 4 * nrx * ntx * ((nr * nr if sides & abi.COV_RX else 0) + (nt * nt if sides & abi.COV_TX else 0))
    a, spec = _arrays(), _spec()
    assert product_lib.hrt_covariance_out_floats(4, 4, None, C.byref(spec)) == 0
    assert product_lib.hrt_covariance_out_floats(4, 4, C.byref(a), None) == 0
    v = abi.covariance_views(np.arange(2 * 3 * 2 * (16 + 4), dtype=np.complex64), 2, 3, 4, 2)
    assert v["rx"].shape == (2, 3, 2, 4, 4) and v["tx"].shape == (2, 3, 2, 2, 2)
    assert v["rx"][0, 0, 0, 0, 1] == 1 and v["tx"][0, 0, 0, 0, 0] == 2 * 3 * 2 * 16
    assert abi.covariance_views(np.zeros(16, np.complex64), 1, 2, 0, 2)["rx"].size == 0


def _drop_in(product_lib, spec, nr=4, nt=3, rx=True, tx=True, fa=3.5e9, cfg=None):
    c = K.small(K.C1, 64) if cfg is None else cfg
    return abi.run_compute_array_covariance(product_lib, *K.args(c), spec, _el(nr) if rx else None,
                                            _el(nt) if tx else None, array_frequency=fa)


@pytest.mark.parametrize("bad", sorted(BAD))
def test_invalid_call_is_refused_by_every_entry(product_lib, bad):
    so, ao, what = BAD[bad]
    spec, a = _spec(**so), _arrays(**ao)
    out = C.c_uint64(7)
    assert product_lib.hrt_array_covariance_scratch_bytes(None, None, C.byref(spec), C.byref(a),
                                                          C.byref(out)) == HRT_E_INVALID
    assert out.value == 7
    assert what.encode() in product_lib.hrt_last_error()
    assert product_lib.hrt_array_covariance(None, None, None, C.byref(spec), C.byref(a), None, 0, None, 0,
                                            None) == HRT_E_INVALID
    msg = product_lib.hrt_last_error()
    assert b"hrt_array_covariance" in msg and what.encode() in msg
    # the drop-in entry refuses it before it creates a problem (no device needed to get the answer)
    with pytest.raises(RuntimeError, match=r"hrt_compute_array_covariance failed \(-1\)"):
        _drop_in(product_lib, spec, ao.get("nr", 4), ao.get("nt", 3), ao.get("rx", PTR) is not None,
                 ao.get("tx", PTR) is not None, ao.get("fa", 3.5e9))
    assert what.encode() in product_lib.hrt_last_error()


def test_null_spec_and_arrays_are_refused(product_lib):
    spec, a = _spec(), _arrays()
    out = C.c_uint64(7)
    L = product_lib
    assert L.hrt_array_covariance_scratch_bytes(None, None, None, C.byref(a), C.byref(out)) == HRT_E_INVALID
    assert b"NULL spec" in L.hrt_last_error()
    assert L.hrt_array_covariance_scratch_bytes(None, None, C.byref(spec), None, C.byref(out)) == HRT_E_INVALID
    assert b"NULL arrays" in L.hrt_last_error()
    assert L.hrt_array_covariance(None, None, None, None, C.byref(a), None, 0, None, 0, None) == HRT_E_INVALID
    assert b"NULL spec" in L.hrt_last_error()
    assert L.hrt_array_covariance(None, None, None, C.byref(spec), None, None, 0, None, 0, None) == HRT_E_INVALID
    assert b"NULL arrays" in L.hrt_last_error()
    assert out.value == 7


def test_offsets_that_are_not_finite_are_refused_by_the_drop_in(product_lib):
    c = K.small(K.C1, 64)
    for side in ("rx", "tx"):
        e = {"rx": _el(4), "tx": _el(3)}
        e[side][1, 2] = math.nan
        with pytest.raises(RuntimeError, match=r"hrt_compute_array_covariance failed \(-1\)"):
            abi.run_compute_array_covariance(product_lib, *K.args(c), _spec(), e["rx"], e["tx"], array_frequency=3.5e9)
        assert (side.upper() + " element 1").encode() in product_lib.hrt_last_error()


def _endpoints(n):
    return [[float(i), 0.0, 1.0] for i in range(n)]


@pytest.mark.parametrize("nrx,ntx,nr,nt,what", [
    (256, 256, 1, 1, "num_rx * num_tx"),
    (64, 64, 256, 256, "2^26"),
    (17, 16, 256, 256, "2^26"),        # 16 x 16 links are exactly 2^26 outputs
])
def test_size_limits_are_refused_by_the_drop_in(product_lib, nrx, ntx, nr, nt, what):
    c = dict(K.small(K.C1, 64))
    c["rx_pos"], c["rx_vel"] = _endpoints(nrx), [[0.0, 0.0, 0.0]] * nrx
    c["tx_pos"], c["tx_vel"] = _endpoints(ntx), [[0.0, 0.0, 0.0]] * ntx
    assert nrx * ntx > 65535 or nrx * ntx * 2 * (nr * nr + nt * nt) > 1 << 26
    with pytest.raises(RuntimeError, match=r"hrt_compute_array_covariance failed \(-1\)"):
        _drop_in(product_lib, _spec(), nr, nt, cfg=c)
    assert what.encode() in product_lib.hrt_last_error()


def test_largest_call_passes_the_checks(product_lib):
    """256 elements a side, one side alone with nothing given for the other, and each part alone pass the checks that
    need no problem (what fails without a problem is the NULL problem)"""
    for so, ao in ((dict(), dict(nr=256, nt=256)), (dict(sides=abi.COV_RX), dict(nt=0, tx=None)),
                   (dict(sides=abi.COV_TX), dict(nr=0, rx=None)), (dict(sides=abi.COV_TX), dict(nr=5000, rx=None)),
                   (dict(parts=abi.CHANNEL_LOS), dict()), (dict(parts=abi.CHANNEL_SCATTER), dict(nr=1, nt=1))):
        spec, a = _spec(**so), _arrays(**ao)
        assert product_lib.hrt_array_covariance_scratch_bytes(None, None, C.byref(spec), C.byref(a),
                                                              None) == HRT_E_INVALID
        assert b"NULL argument" in product_lib.hrt_last_error(), (so, ao)


def _pybind():
    import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    return hermespy_rt


PYBIND_BAD = {
    "no_parts": (dict(los=False, scatter=False), "parts"),
    "no_sides": (dict(rx_elements=None, tx_elements=None), "sides"),
    "rx_zero_elements": (dict(rx_elements=np.zeros((0, 3), np.float32)), "num_rx_elements"),
    "tx_over_256": (dict(tx_elements=np.zeros((257, 3), np.float32)), "num_tx_elements"),
    "fa_zero": (dict(array_frequency=0.0), "array frequency"),
    "fa_nan": (dict(array_frequency=math.nan), "array frequency"),
    "rx_not_finite": (dict(rx_elements=np.array([[0, 0, 0], [0, math.inf, 0]], np.float32)), "RX element 1"),
}


@pytest.mark.parametrize("bad", sorted(PYBIND_BAD))
def test_pybind_refuses_invalid_call(bad):
    hermespy_rt = _pybind()
    c = K.small(K.C1, 64)
    args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], 1, 1, 64, 1)
    kw = dict(rx_elements=_el(4), tx_elements=_el(3))
    over, what = PYBIND_BAD[bad]
    kw.update(over)
    with pytest.raises(ValueError, match=what):
        hermespy_rt.compute_array_covariance(*args, **kw)


def test_pybind_refuses_the_link_limit():
    hermespy_rt = _pybind()
    c = K.small(K.C1, 64)
    n = 256
    pos, vel = np.array(_endpoints(n), np.float32), np.zeros((n, 3), np.float32)
    with pytest.raises(ValueError, match=r"num_rx \* num_tx"):
        hermespy_rt.compute_array_covariance(c["scene_path"], pos, pos, vel, vel, c["f_ghz"], n, n, 64, 1,
                                             rx_elements=_el(2))


def test_compute_array_covariance_without_device_fails_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny call
    succeeds and returns finite Hermitian matrices.)"""
    if _have_gpu():
        d = _drop_in(product_lib, _spec())
        assert d["rx"].shape == (1, 1, 2, 4, 4) and d["tx"].shape == (1, 1, 2, 3, 3)
        assert np.isfinite(d["buffer"].view(np.float32)).all()
        assert np.array_equal(d["rx"], d["rx"].conj().swapaxes(-1, -2))
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_array_covariance failed \(-3\)") as e:
        _drop_in(product_lib, _spec())
    assert "HIP" in str(e.value)
