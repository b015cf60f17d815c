"""Argument checks of the dominant paths entries (hrt_dominant_out_bytes, hrt_dominant_paths_scratch_bytes,
hrt_dominant_paths, hrt_compute_dominant_paths, hermespy_rt.compute_dominant_paths): a refused spec returns
HRT_E_INVALID before the device is touched, so these run without a GPU.  Without a device a valid call fails loudly
(HRT_E_HIP), never with a CPU result."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi, lib

from . import configs as K

HRT_E_INVALID, HRT_E_HIP = -1, -3
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hrt_dominant_out_bytes", "hrt_dominant_paths_scratch_bytes", "hrt_dominant_paths",
       "hrt_compute_dominant_paths")

# name -> (spec arguments, what the message names)
BAD_SPECS = {
    "no_paths": (dict(max_paths=0), "max_paths"),
    "paths_over_1024": (dict(max_paths=1025), "max_paths"),
    "no_parts": (dict(parts=0), "parts"),
    "unknown_part": (dict(parts=abi.CHANNEL_SCATTER | 4), "parts"),
}


def _spec(max_paths=64, parts=abi.CHANNEL_LOS | abi.CHANNEL_SCATTER):
    return abi.dominant_spec(max_paths, parts=parts)


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def test_structs_match_c(tmp_path):
    spec_fields = ["max_paths", "parts"]
    path_fields = ["power", "path", "bounce", "tri", "a_te_re", "a_te_im", "a_tm_re", "a_tm_im", "tau", "freq_shift",
                   "u_rx", "u_tx"]
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hrt_device.h"\n'
                    'int main(void){printf("%zu' + ' %zu' * (len(spec_fields) + 1 + len(path_fields)) +
                    '\\n", sizeof(hrt_dominant_spec)' +
                    "".join(", offsetof(hrt_dominant_spec, %s)" % f for f in spec_fields) +
                    ", sizeof(hrt_dominant_path)" +
                    "".join(", offsetof(hrt_dominant_path, %s)" % f for f in path_fields) + ');return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    S, P = abi.DominantSpec, abi.DominantPath
    assert got == ([C.sizeof(S)] + [getattr(S, f).offset for f in spec_fields] +
                   [C.sizeof(P)] + [getattr(P, f).offset for f in path_fields])
    assert C.sizeof(P) == 72


def test_views_address_the_struct_fields():
    """dominant_views of a buffer written through the ctypes mirror: every view reads its field, without a copy"""
    nrx, ntx, k = 2, 3, 5
    buf = np.zeros(nrx * ntx * (16 + 72 * k), np.uint8)
    recs = (abi.DominantPath * (nrx * ntx * k)).from_buffer(buf, 16 * nrx * ntx)
    for n, r in enumerate(recs):
        r.power, r.path, r.bounce, r.tri = n + 0.5, (1 << 40) + n, n - 1, 7 * n
        r.a_te_re, r.a_te_im, r.a_tm_re, r.a_tm_im, r.tau, r.freq_shift = n + 1, n + 2, n + 3, n + 4, n + 5, n + 6
        r.u_rx[:] = [n + 7, n + 8, n + 9]
        r.u_tx[:] = [n + 10, n + 11, n + 12]
    buf[:16 * nrx * ntx].view(np.uint64)[:] = np.arange(2 * nrx * ntx)
    v = abi.dominant_views(buf, nrx, ntx, k)
    n = np.arange(nrx * ntx * k).reshape(nrx, ntx, k)
    assert np.array_equal(v["kept"].ravel(), np.arange(0, 12, 2)) and np.array_equal(v["eligible"].ravel(),
                                                                                      np.arange(1, 12, 2))
    assert np.array_equal(v["power"], n + 0.5) and np.array_equal(v["path"], (1 << 40) + n)
    assert np.array_equal(v["bounce"], n - 1) and np.array_equal(v["tri"], 7 * n)
    assert np.array_equal(v["a_te"], (n + 1) + 1j * (n + 2)) and np.array_equal(v["a_tm"], (n + 3) + 1j * (n + 4))
    assert np.array_equal(v["tau"], n + 5) and np.array_equal(v["freq_shift"], n + 6)
    assert np.array_equal(v["u_rx"], n[..., None] + np.arange(7, 10))
    assert np.array_equal(v["u_tx"], n[..., None] + np.arange(10, 13))
    assert v["path"].dtype == np.uint64 and v["bounce"].dtype == np.int32 and v["a_te"].dtype == np.complex64
    for name, a in v.items():
        assert np.shares_memory(a, buf), name
    import torch
    t = abi.dominant_views(torch.from_numpy(buf), nrx, ntx, k)
    for name in v:
        assert np.array_equal(t[name].numpy().view(v[name].dtype), v[name]), name
        assert t[name].data_ptr() == v[name].__array_interface__["data"][0], name


def test_out_bytes(product_lib):
    for nrx, ntx, k in ((1, 1, 1), (3, 5, 64), (8, 8, 1024), (64, 64, 1024)):
        spec = _spec(k)
        want = nrx * ntx * (16 + 72 * k)
        assert product_lib.hrt_dominant_out_bytes(nrx, ntx, C.byref(spec)) == want
        assert abi.dominant_out_bytes(nrx, ntx, spec) == want
    assert product_lib.hrt_dominant_out_bytes(4, 4, None) == 0
    for nrx, ntx, spec in ((1, 1, _spec(0)), (1, 1, _spec(1025)), (1, 1, _spec(parts=0)), (256, 256, _spec(1)),
                           (64, 65, _spec(1024))):
        assert product_lib.hrt_dominant_out_bytes(nrx, ntx, C.byref(spec)) == 0
        assert abi.dominant_out_bytes(nrx, ntx, spec) == 0


@pytest.mark.parametrize("bad", sorted(BAD_SPECS))
def test_invalid_spec_is_refused_by_every_entry(product_lib, bad):
    over, what = BAD_SPECS[bad]
    spec = _spec(**over)
    out = C.c_uint64(7)
    assert product_lib.hrt_dominant_paths_scratch_bytes(None, None, C.byref(spec), C.byref(out)) == HRT_E_INVALID
    assert out.value == 7
    assert what.encode() in product_lib.hrt_last_error()
    assert product_lib.hrt_dominant_paths(None, None, None, C.byref(spec), None, 0, None, 0, None) == HRT_E_INVALID
    assert b"hrt_dominant_paths" in product_lib.hrt_last_error()
    assert what.encode() in product_lib.hrt_last_error()
    # the drop-in entry refuses it before it creates a problem (no device needed to get the answer)
    with pytest.raises(RuntimeError, match=r"hrt_compute_dominant_paths failed \(-1\)"):
        abi.run_compute_dominant_paths(product_lib, *K.args(K.small(K.C1, 64)), spec)
    assert what.encode() in product_lib.hrt_last_error()


def test_null_spec_is_refused(product_lib):
    out = C.c_uint64(7)
    assert product_lib.hrt_dominant_paths_scratch_bytes(None, None, None, C.byref(out)) == HRT_E_INVALID
    assert b"NULL spec" in product_lib.hrt_last_error() and out.value == 7
    assert product_lib.hrt_dominant_paths(None, None, None, None, None, 0, None, 0, None) == HRT_E_INVALID
    assert b"NULL spec" in product_lib.hrt_last_error()
    assert product_lib.hrt_compute_dominant_paths(None, None, None, None, None, C.c_float(3.0), 1, 1, 64, 1, None,
                                                  None, None) == HRT_E_INVALID
    assert b"NULL spec" in product_lib.hrt_last_error()


def _endpoints(n):
    return [[float(i), 0.0, 1.0] for i in range(n)]


def _many(nrx, ntx):
    c = dict(K.small(K.C1, 64))
    c["rx_pos"], c["rx_vel"] = _endpoints(nrx), [[0.0, 0.0, 0.0]] * nrx
    c["tx_pos"], c["tx_vel"] = _endpoints(ntx), [[0.0, 0.0, 0.0]] * ntx
    return c


LINK_LIMITS = [(256, 256, 1, "num_rx * num_tx = 65536 > 65535"), (64, 65, 1024, "num_rx * num_tx * max_paths"),
               (4097, 1, 1024, "2^22")]


@pytest.mark.parametrize("nrx,ntx,k,what", LINK_LIMITS)
def test_link_limits_are_refused_by_the_drop_in(product_lib, nrx, ntx, k, what):
    buf = np.zeros(16, np.uint8)   # (never written: the call is refused first)
    scene = product_lib.scene_load(str(K.C1["scene_path"]).encode())
    c = _many(nrx, ntx)
    V3 = C.POINTER(abi.Vec3)
    a = [np.ascontiguousarray(np.asarray(c[k_], np.float32)) for k_ in ("rx_pos", "tx_pos", "rx_vel", "tx_vel")]
    spec = _spec(k)
    try:
        rc = product_lib.hrt_compute_dominant_paths(C.byref(scene), *[x.ctypes.data_as(V3) for x in a], C.c_float(3.0),
                                                    nrx, ntx, 64, 1, C.byref(spec), buf.ctypes.data_as(C.c_void_p),
                                                    None)
    finally:
        abi.free_scene(scene)
    assert rc == HRT_E_INVALID
    assert what.encode() in product_lib.hrt_last_error()


def test_largest_spec_passes_the_spec_check(product_lib):
    """K = 1 and K = 1024 and the LoS / scatter parts alone pass the spec check (what fails without a problem is the
    NULL problem)"""
    for spec in (_spec(1), _spec(1024), _spec(parts=abi.CHANNEL_LOS), _spec(parts=abi.CHANNEL_SCATTER)):
        assert product_lib.hrt_dominant_paths_scratch_bytes(None, None, C.byref(spec), None) == HRT_E_INVALID
        assert b"NULL" in product_lib.hrt_last_error() and b"spec" not in product_lib.hrt_last_error()


def test_new_entries_are_exported_and_declared(product_lib):
    exports = open(os.path.join(REPO, "hermespy-rt_amd", "csrc", "exports.map")).read()
    device_h = open(os.path.join(REPO, "include", "hrt_device.h")).read()
    public_h = open(os.path.join(REPO, "include", "hermespy_rt.h")).read()
    for name in NEW:
        assert name in lib.EXPORTED
        assert re.search(r"\b%s;" % name, exports), name
        assert getattr(product_lib, name).argtypes is not None, name
    for name in ("hrt_dominant_paths_scratch_bytes", "hrt_dominant_paths"):
        assert re.search(r"\bint %s\(" % name, device_h), name
    for name in ("hrt_dominant_out_bytes", "hrt_compute_dominant_paths", "hrt_dominant_spec", "hrt_dominant_path"):
        assert re.search(r"\b%s\b" % name, public_h), name
    # both meanings of `tri` are stated
    assert "ROW of the device table" in device_h and "flat index" in public_h


def _pybind():
    import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    return hermespy_rt


PYBIND_BAD = {
    "no_paths": (1, 1, dict(max_paths=0), "max_paths"),
    "paths_over_1024": (1, 1, dict(max_paths=1025), "max_paths"),
    "paths_over_32_bits": (1, 1, dict(max_paths=1 << 33), "32 bits"),
    "no_parts": (1, 1, dict(max_paths=4, los=False, scatter=False), "parts"),
    "links_over_65535": (256, 256, dict(max_paths=1), "num_rx \\* num_tx"),
    "link_paths_over_2_22": (64, 65, dict(max_paths=1024), "2\\^22"),
}


@pytest.mark.parametrize("bad", sorted(PYBIND_BAD))
def test_pybind_refuses_invalid_spec(bad):
    hermespy_rt = _pybind()
    nrx, ntx, kw, what = PYBIND_BAD[bad]
    c = _many(nrx, ntx)
    args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
            np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], nrx, ntx, 64, 1)
    with pytest.raises(ValueError, match=what):
        hermespy_rt.compute_dominant_paths(*args, **kw)


def test_compute_dominant_paths_without_device_fails_loudly(product_lib):
    """no HIP device: HRT_E_HIP and a message naming HIP -- never a CPU result.  (On a GPU box the same tiny call
    succeeds and returns a sorted list.)"""
    c = K.small(K.C1, 64)
    if _have_gpu():
        d = abi.run_compute_dominant_paths(product_lib, *K.args(c), _spec(8))
        kept = int(d["kept"][0, 0])
        assert d["power"].shape == (1, 1, 8) and 0 < kept <= min(8, int(d["eligible"][0, 0]))
        assert (np.diff(d["power"][0, 0, :kept]) <= 0).all() and not d["buffer"][16 + 72 * kept:].any()
        return
    with pytest.raises(RuntimeError, match=r"hrt_compute_dominant_paths failed \(-3\)") as e:
        abi.run_compute_dominant_paths(product_lib, *K.args(c), _spec())
    assert "HIP" in str(e.value)
