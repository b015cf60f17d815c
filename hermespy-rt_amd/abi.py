"""ctypes mirror of the reference's C ABI for the compute_paths hot path.

This is the host-side (Python) statement of the drop-in boundary.  Every struct below is
byte-compatible with the reference header it cites, so driver code written against these
declarations works with any library that exports the reference's three entry points -- the
product loads its own (lib.py); tests/ use the same declarations to drive the checker builds.

Reference interface mirrored here:
  Vec3            inc/vec3.h:6-8
  Ray             inc/ray.h:6-9
  Mesh, Scene     inc/scene.h:10-32
  ChannelInfo     inc/compute_paths.h:13-23
  RaysInfo        inc/compute_paths.h:26-30
  compute_paths   inc/compute_paths.h:59-74
  scene_load      inc/scene.h:105   (returns Scene BY VALUE)
  scene_save      inc/scene.h:95
"""
import ctypes as C

import numpy as np

c_float_p = C.POINTER(C.c_float)


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Ray(C.Structure):
    _fields_ = [("o", Vec3), ("d", Vec3)]


class Mesh(C.Structure):
    _fields_ = [
        ("num_vertices", C.c_uint32),
        ("vs", C.POINTER(Vec3)),
        ("num_triangles", C.c_uint32),
        ("is_", C.POINTER(C.c_uint32)),
        ("material_index", C.c_uint32),
        ("velocity", Vec3),
        ("ns", C.POINTER(Vec3)),
    ]


class Scene(C.Structure):
    _fields_ = [("num_meshes", C.c_uint32), ("meshes", C.POINTER(Mesh))]


class ChannelInfo(C.Structure):
    _fields_ = [
        ("num_rays", C.c_uint32),
        ("directions_rx", C.POINTER(Vec3)),
        ("directions_tx", C.POINTER(Vec3)),
        ("a_te_re", c_float_p),
        ("a_te_im", c_float_p),
        ("a_tm_re", c_float_p),
        ("a_tm_im", c_float_p),
        ("tau", c_float_p),
        ("freq_shift", c_float_p),
    ]


class RaysInfo(C.Structure):
    _fields_ = [
        ("num_bounces", C.c_uint32),
        ("num_rays", C.c_uint32),
        ("rays", C.POINTER(Ray)),
        ("rays_active", C.POINTER(C.c_uint8)),
    ]


assert C.sizeof(Vec3) == 12 and C.sizeof(Ray) == 24
assert C.sizeof(Mesh) == 56 and C.sizeof(Scene) == 16
assert C.sizeof(ChannelInfo) == 72 and C.sizeof(RaysInfo) == 24

#: bit pattern used to pre-fill every output buffer so "slot not written" is observable
#: (the reference leaves slots of dead rays untouched).
SENTINEL_U32 = 0x7FC0DEAD


def bind_c_abi(lib):
    """Declare argtypes/restype of compute_paths / scene_load / scene_save (the reference's
    signatures, inc/compute_paths.h:59-74, inc/scene.h:95-105) on the loaded library `lib`."""
    lib.scene_load.argtypes = [C.c_char_p]
    lib.scene_load.restype = Scene
    lib.scene_save.argtypes = [C.POINTER(Scene), C.c_char_p]
    lib.scene_save.restype = None
    lib.compute_paths.argtypes = [
        C.POINTER(Scene),
        C.POINTER(Vec3), C.POINTER(Vec3), C.POINTER(Vec3), C.POINTER(Vec3),
        C.c_float,
        C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
        C.POINTER(ChannelInfo), C.POINTER(RaysInfo),
        C.POINTER(ChannelInfo), C.POINTER(RaysInfo),
    ]
    lib.compute_paths.restype = None
    return lib


def _sentinel(n, dtype=np.float32):
    if dtype == np.uint8:
        return np.full(n, 0xAD, dtype=np.uint8)
    return np.full(n, SENTINEL_U32, dtype=np.uint32).view(np.float32)


def _vec3_arg(a, n):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(n, 3))
    return a, a.ctypes.data_as(C.POINTER(Vec3))


def free_scene(scene):
    """inc/scene.h:72-86 (static inline in the reference header; uses free())."""
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    for i in range(scene.num_meshes):
        m = scene.meshes[i]
        for p in (m.vs, m.is_, m.ns):
            libc.free(C.cast(p, C.c_void_p))
    libc.free(C.cast(scene.meshes, C.c_void_p))


def scene_to_numpy(scene):
    """Deep-copy a loaded Scene into python lists of numpy arrays (for inspection/tests)."""
    out = []
    for i in range(scene.num_meshes):
        m = scene.meshes[i]
        vs = np.ctypeslib.as_array(C.cast(m.vs, c_float_p), shape=(m.num_vertices, 3)).copy()
        idx = np.ctypeslib.as_array(m.is_, shape=(m.num_triangles, 3)).copy()
        ns = None
        if m.ns:
            ns = np.ctypeslib.as_array(C.cast(m.ns, c_float_p), shape=(m.num_triangles, 3)).copy()
        out.append(dict(vs=vs, idx=idx, material_index=int(m.material_index),
                        velocity=np.array([m.velocity.x, m.velocity.y, m.velocity.z], np.float32),
                        ns=ns))
    return out


def run_compute_paths(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths,
                      num_bounces, zero_freq_shift=None, with_rays=True, stats=None, interleaved=False):
    """Call `lib.compute_paths` the way the reference's own callers do
    (compute_paths_pybind11.cpp:99-186, test/test.c:10-75) and return every output as numpy.

    All outputs are pre-filled with SENTINEL_U32 so unwritten slots are visible.  The scatter
    freq_shift is zero-filled when num_tx > 1 (the reference memcpy-replicates caller memory
    there) unless `zero_freq_shift` overrides.  rays_active is allocated with
    the size the callee really needs, (ntx*nb+1)*(np/8+1).
    """
    rx_pos = np.asarray(rx_pos, np.float32).reshape(-1, 3)
    tx_pos = np.asarray(tx_pos, np.float32).reshape(-1, 3)
    nrx, ntx = rx_pos.shape[0], tx_pos.shape[0]
    npth, nb = int(num_paths), int(num_bounces)
    rxp, rxp_c = _vec3_arg(rx_pos, nrx)
    txp, txp_c = _vec3_arg(tx_pos, ntx)
    rxv, rxv_c = _vec3_arg(rx_vel, nrx)
    txv, txv_c = _vec3_arg(tx_vel, ntx)

    def chan(n, n_dir_tx):
        d = dict(directions_rx=_sentinel(3 * n), directions_tx=_sentinel(3 * n_dir_tx),
                 a_te_re=_sentinel(n), a_te_im=_sentinel(n), a_tm_re=_sentinel(n),
                 a_tm_im=_sentinel(n), tau=_sentinel(n), freq_shift=_sentinel(n))
        ci = ChannelInfo()
        if interleaved:
            # hrt_compute_paths_interleaved: re and im of one polarisation share an array of 2 n floats
            # (what a complex64 array is); the result dict still shows them as two (strided) planes
            for pol in ("a_te", "a_tm"):
                both = _sentinel(2 * n)
                d[pol + "_both"] = both
                d[pol + "_re"], d[pol + "_im"] = both[0::2], both[1::2]
        for k, v in d.items():
            if k.endswith("_both"):
                continue
            ptr_t = C.POINTER(Vec3) if k.startswith("directions") else c_float_p
            if interleaved and k in ("a_te_re", "a_te_im", "a_tm_re", "a_tm_im"):
                base = d[k[:4] + "_both"].ctypes.data + (4 if k.endswith("_im") else 0)
                setattr(ci, k, C.cast(base, c_float_p))
            else:
                setattr(ci, k, v.ctypes.data_as(ptr_t))
        return d, ci

    n_los = nrx * ntx
    n_scat = nrx * ntx * nb * npth
    los, los_c = chan(n_los, n_los)
    scat, scat_c = chan(n_scat, n_scat)
    los_c.num_rays = 1
    scat_c.num_rays = (nb * npth) & 0xFFFFFFFF
    if zero_freq_shift is None:
        zero_freq_shift = ntx > 1
    if zero_freq_shift:
        scat["freq_shift"][:] = 0.0

    los_rays = _sentinel(6 * n_los)
    los_active = _sentinel(n_los // 8 + 1, np.uint8)
    n_rays_scat = ntx * (nb + 1) * npth
    n_act_scat = (ntx * nb + 1) * (npth // 8 + 1)
    scat_rays = _sentinel(6 * n_rays_scat)
    scat_active = _sentinel(n_act_scat, np.uint8)
    lr = RaysInfo(1, 1, los_rays.ctypes.data_as(C.POINTER(Ray)),
                  los_active.ctypes.data_as(C.POINTER(C.c_uint8)))
    sr = RaysInfo(nb + 1, npth & 0xFFFFFFFF, scat_rays.ctypes.data_as(C.POINTER(Ray)),
                  scat_active.ctypes.data_as(C.POINTER(C.c_uint8)))

    scene = lib.scene_load(str(scene_path).encode())
    try:
        if stats is not None or not with_rays or interleaved:
            # product-only entry points: status code, optional RaysInfo, counters
            entry = lib.hrt_compute_paths_interleaved if interleaved else lib.hrt_compute_paths_ex
            rc = entry(C.byref(scene), rxp_c, txp_c, rxv_c, txv_c,
                                          C.c_float(f_ghz), nrx, ntx, npth, nb, C.byref(los_c),
                                          C.byref(lr) if with_rays else None, C.byref(scat_c),
                                          C.byref(sr) if with_rays else None,
                                          C.byref(stats) if stats is not None else None)
            if rc != 0:
                raise RuntimeError("hrt_compute_paths_ex failed (%d): %s" % (rc, lib.hrt_last_error().decode()))
        else:
            lib.compute_paths(C.byref(scene), rxp_c, txp_c, rxv_c, txv_c, C.c_float(f_ghz),
                              nrx, ntx, npth, nb, C.byref(los_c), C.byref(lr),
                              C.byref(scat_c), C.byref(sr))
        normals = [m["ns"] for m in scene_to_numpy(scene)]
    finally:
        free_scene(scene)

    shp = (nrx, ntx, nb, npth)
    los = {k: v for k, v in los.items() if not k.endswith("_both")}
    scat = {k: v for k, v in scat.items() if not k.endswith("_both")}
    res = dict(
        los={k: (v.reshape(nrx, ntx, 3) if k.startswith("directions") else v.reshape(nrx, ntx))
             for k, v in los.items()},
        scat={k: (v.reshape(*shp, 3) if k.startswith("directions") else v.reshape(shp))
              for k, v in scat.items()},
        los_rays=los_rays.reshape(n_los, 6), los_active=los_active,
        scat_rays=scat_rays.reshape(n_rays_scat, 6), scat_active=scat_active,
        normals=normals,
    )
    return res


def written(a):
    """Boolean mask of slots whose bit pattern is not the sentinel."""
    return a.view(np.uint32) != SENTINEL_U32


class PathList(C.Structure):
    """include/hermespy_rt.h hrt_path_list"""
    _fields_ = [
        ("num", C.c_uint64), ("num_rx", C.c_uint32), ("num_tx", C.c_uint32),
        ("rx", C.POINTER(C.c_uint32)), ("tx", C.POINTER(C.c_uint32)), ("bounce", C.POINTER(C.c_uint32)),
        ("path", C.POINTER(C.c_uint64)),
        ("a_te_re", c_float_p), ("a_te_im", c_float_p), ("a_tm_re", c_float_p), ("a_tm_im", c_float_p),
        ("tau", c_float_p), ("direction_rx", C.POINTER(Vec3)), ("freq_shift", c_float_p),
        ("unblocked", C.POINTER(C.c_uint8)), ("mesh", C.POINTER(C.c_uint32)), ("face", C.POINTER(C.c_uint32)),
        ("los", c_float_p),
    ]


def run_compute_paths_list(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths,
                           num_bounces, include_blocked=False, stats=None):
    """hrt_compute_paths_list through ctypes -> dict of numpy arrays (copies; the C list is freed)."""
    rx_pos = np.asarray(rx_pos, np.float32).reshape(-1, 3)
    tx_pos = np.asarray(tx_pos, np.float32).reshape(-1, 3)
    nrx, ntx = rx_pos.shape[0], tx_pos.shape[0]
    _, rxp = _vec3_arg(rx_pos, nrx)
    _, txp = _vec3_arg(tx_pos, ntx)
    rxv_a, rxv = _vec3_arg(rx_vel, nrx)
    txv_a, txv = _vec3_arg(tx_vel, ntx)
    lib.hrt_compute_paths_list.restype = C.c_int
    lib.hrt_path_list_free.restype = None
    pl = PathList()
    scene = lib.scene_load(str(scene_path).encode())
    try:
        rc = lib.hrt_compute_paths_list(C.byref(scene), rxp, txp, rxv, txv, C.c_float(f_ghz),
                                        C.c_size_t(nrx), C.c_size_t(ntx), C.c_size_t(int(num_paths)),
                                        C.c_size_t(int(num_bounces)), C.c_int(1 if include_blocked else 0),
                                        C.byref(pl), C.byref(stats) if stats is not None else None)
        if rc != 0:
            raise RuntimeError("hrt_compute_paths_list failed (%d): %s" % (rc, lib.hrt_last_error().decode()))
        n = int(pl.num)

        def arr(ptr, dtype, shape):
            if n == 0:
                return np.zeros(shape, dtype)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)),
                                         shape=(int(np.prod(shape)) * np.dtype(dtype).itemsize,)).view(dtype).reshape(shape).copy()

        out = dict(rx=arr(pl.rx, np.uint32, (n,)), tx=arr(pl.tx, np.uint32, (n,)),
                   bounce=arr(pl.bounce, np.uint32, (n,)), path=arr(pl.path, np.uint64, (n,)),
                   tau=arr(pl.tau, np.float32, (n,)), direction_rx=arr(pl.direction_rx, np.float32, (n, 3)),
                   freq_shift=arr(pl.freq_shift, np.float32, (n,)), unblocked=arr(pl.unblocked, np.uint8, (n,)).astype(bool),
                   mesh=arr(pl.mesh, np.uint32, (n,)), face=arr(pl.face, np.uint32, (n,)))
        for k in ("a_te_re", "a_te_im", "a_tm_re", "a_tm_im"):
            out[k] = arr(getattr(pl, k), np.float32, (n,))
        out["los"] = np.ctypeslib.as_array(pl.los, shape=(nrx * ntx * 8,)).copy().reshape(nrx, ntx, 8)
    finally:
        lib.hrt_path_list_free(C.byref(pl))
        free_scene(scene)
    return out


CHANNEL_LOS, CHANNEL_SCATTER = 1, 2   # hrt_channel_spec.parts


class ChannelSpec(C.Structure):
    """include/hermespy_rt.h hrt_channel_spec"""
    _fields_ = [("f0_hz", C.c_double), ("df_hz", C.c_double), ("num_freqs", C.c_uint32),
                ("t0_s", C.c_double), ("dt_s", C.c_double), ("num_times", C.c_uint32),
                ("parts", C.c_uint32)]


def channel_spec(f0, df, num_freqs, t0=0.0, dt=0.0, num_times=1, los=True, scatter=True, parts=None):
    if parts is None:
        parts = (CHANNEL_LOS if los else 0) | (CHANNEL_SCATTER if scatter else 0)
    return ChannelSpec(float(f0), float(df), int(num_freqs), float(t0), float(dt), int(num_times), int(parts))


def _run_pathsum(lib, name, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                 out_shape, extra, stats, dtype=np.complex64):
    """One of the nine path-sum drop-in entries (`name`: hrt_compute_channel, _array_channel, _taps, _array_taps,
    _power_profiles, _dominant_paths, _beam_channel, _beam_taps or _array_covariance) or hrt_compute_received_signal
    through ctypes, into a numpy array
    of `dtype` and shape (nrx, ntx) + out_shape (a flat buffer of out_shape doubles for float64, floats for float32 or
    bytes for uint8; out_shape None: a placeholder the library
    refuses to write); `extra` are the arguments that follow the spec.  Raises RuntimeError("<name> failed (<rc>): ...") on an error code."""
    rx_pos = np.asarray(rx_pos, np.float32).reshape(-1, 3)
    tx_pos = np.asarray(tx_pos, np.float32).reshape(-1, 3)
    nrx, ntx = rx_pos.shape[0], tx_pos.shape[0]
    _, rxp = _vec3_arg(rx_pos, nrx)
    _, txp = _vec3_arg(tx_pos, ntx)
    rxv_a, rxv = _vec3_arg(rx_vel, nrx)
    txv_a, txv = _vec3_arg(tx_vel, ntx)
    if out_shape is None:
        out_shape = (1,)
    elif dtype == np.complex64:
        out_shape = (nrx, ntx) + tuple(out_shape)
    out = np.zeros(out_shape, dtype)
    scene = lib.scene_load(str(scene_path).encode())
    try:
        rc = getattr(lib, name)(C.byref(scene), rxp, txp, rxv, txv, C.c_float(f_ghz), C.c_size_t(nrx), C.c_size_t(ntx),
                                C.c_size_t(int(num_paths)), C.c_size_t(int(num_bounces)), C.byref(spec), *extra,
                                out.ctypes.data_as(C.c_void_p if dtype == np.uint8 else
                                                   C.POINTER(C.c_double if dtype == np.float64 else C.c_float)),
                                C.byref(stats) if stats is not None else None)
    finally:
        free_scene(scene)
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (name, rc, lib.hrt_last_error().decode()))
    return out


def run_compute_channel(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                        stats=None):
    """hrt_compute_channel through ctypes -> complex64 [nrx, ntx, 2, num_times, num_freqs].  Raises
    RuntimeError("hrt_compute_channel failed (<rc>): ...") on an error code."""
    shape = (2, max(int(spec.num_times), 1), max(int(spec.num_freqs), 1))
    return _run_pathsum(lib, "hrt_compute_channel", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths,
                        num_bounces, spec, shape, (), stats)

class ArraySpec(C.Structure):
    """include/hrt_device.h hrt_array_spec (the element pointers are device pointers)"""
    _fields_ = [("num_rx_elements", C.c_uint32), ("num_tx_elements", C.c_uint32),
                ("rx_elements", C.c_void_p), ("tx_elements", C.c_void_p), ("array_frequency_hz", C.c_double)]


def elements(e, name):
    """element offsets as a contiguous float32 [n, 3] numpy array (n >= 0; the library checks the limits)"""
    a = np.ascontiguousarray(np.asarray(e, np.float32))
    if a.ndim == 1 and a.size == 3:
        a = a.reshape(1, 3)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s must have shape (n, 3), got %s" % (name, a.shape))
    return a


def _array_args(rx_elements, tx_elements, f_ghz, array_frequency):
    """-> Nr, Nt and the arguments that follow the spec of hrt_compute_array_channel / _array_taps (array_frequency
    defaults to the carrier)"""
    re, te = elements(rx_elements, "rx_elements"), elements(tx_elements, "tx_elements")
    nr, nt = re.shape[0], te.shape[0]
    V3 = C.POINTER(Vec3)
    fa = float(f_ghz) * 1e9 if array_frequency is None else float(array_frequency)
    return nr, nt, (re.ctypes.data_as(V3), C.c_size_t(nr), te.ctypes.data_as(V3), C.c_size_t(nt), C.c_double(fa))


def run_compute_array_channel(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                              rx_elements, tx_elements, array_frequency=None, stats=None):
    """hrt_compute_array_channel through ctypes -> complex64 [nrx, ntx, Nr, Nt, 2, num_times, num_freqs]
    (array_frequency defaults to the carrier).  Raises RuntimeError("hrt_compute_array_channel failed (<rc>): ...")
    on an error code."""
    nr, nt, extra = _array_args(rx_elements, tx_elements, f_ghz, array_frequency)
    # (an output too large for the host is refused by the library's limits first: allocate only what passes them)
    pts = nr * nt * int(spec.num_times) * int(spec.num_freqs)
    shape = (max(nr, 1), max(nt, 1), 2, max(int(spec.num_times), 1), max(int(spec.num_freqs), 1))
    return _run_pathsum(lib, "hrt_compute_array_channel", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths,
                        num_bounces, spec, shape if 0 < pts <= (1 << 24) else None, extra, stats)

class BeamSpec(C.Structure):
    """include/hrt_device.h hrt_beam_spec (the weight pointers are device pointers)"""
    _fields_ = [("num_rx_beams", C.c_uint32), ("num_tx_beams", C.c_uint32),
                ("rx_weights", C.c_void_p), ("tx_weights", C.c_void_p)]


def weights(w, n_elements, name):
    """a codebook as a contiguous complex64 [beams, n_elements] numpy array (beams >= 0; the library checks the
    limits): one row per beam; a 1-D array of n_elements weights is one beam"""
    a = np.asarray(w)
    if a.dtype.kind not in "fc":
        raise ValueError("%s must be a real or complex floating-point array, got %s" % (name, a.dtype))
    a = np.ascontiguousarray(a, np.complex64)
    if a.ndim == 1 and a.size == n_elements:
        a = a.reshape(1, n_elements)
    if a.ndim != 2 or a.shape[1] != n_elements:
        raise ValueError("%s must have shape (beams, %d), got %s" % (name, n_elements, a.shape))
    return a


def run_compute_beam_channel(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                             rx_elements, tx_elements, rx_weights, tx_weights, array_frequency=None, stats=None):
    """hrt_compute_beam_channel through ctypes -> complex64 [nrx, ntx, Br, Bt, 2, num_times, num_freqs]: rx_weights
    (Br, Nr) is applied conjugated (the combiner w^H), tx_weights (Bt, Nt) as it is; array_frequency defaults to the
    carrier.  Raises RuntimeError("hrt_compute_beam_channel failed (<rc>): ...") on an error code."""
    nr, nt, extra = _array_args(rx_elements, tx_elements, f_ghz, array_frequency)
    wr, wt = weights(rx_weights, nr, "rx_weights"), weights(tx_weights, nt, "tx_weights")
    br, bt = wr.shape[0], wt.shape[0]
    extra += (wr.ctypes.data_as(c_float_p), C.c_size_t(br), wt.ctypes.data_as(c_float_p), C.c_size_t(bt))
    # (an output too large for the host is refused by the library's limits first: allocate only what passes them)
    pts = br * bt * int(spec.num_times) * int(spec.num_freqs)
    shape = (br, bt, 2, int(spec.num_times), int(spec.num_freqs))
    return _run_pathsum(lib, "hrt_compute_beam_channel", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths,
                        num_bounces, spec, shape if 0 < pts <= (1 << 24) else None, extra, stats)


class TapsSpec(C.Structure):
    """include/hermespy_rt.h hrt_taps_spec"""
    _fields_ = [("fs_hz", C.c_double), ("fc_hz", C.c_double), ("t0_s", C.c_double), ("dt_s", C.c_double),
                ("l_min", C.c_int32), ("num_taps", C.c_uint32), ("num_times", C.c_uint32), ("parts", C.c_uint32)]


def taps_spec(fs, num_taps, l_min=0, fc=0.0, t0=0.0, dt=0.0, num_times=1, los=True, scatter=True, parts=None):
    if parts is None:
        parts = (CHANNEL_LOS if los else 0) | (CHANNEL_SCATTER if scatter else 0)
    return TapsSpec(float(fs), float(fc), float(t0), float(dt), int(l_min), int(num_taps), int(num_times), int(parts))


def run_compute_taps(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                     stats=None):
    """hrt_compute_taps through ctypes -> complex64 [nrx, ntx, 2, num_times, num_taps].  Raises
    RuntimeError("hrt_compute_taps failed (<rc>): ...") on an error code."""
    # (an output too large for the host is refused by the library's limits first: allocate only what passes them)
    nt, nl = int(spec.num_times), int(spec.num_taps)
    return _run_pathsum(lib, "hrt_compute_taps", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths,
                        num_bounces, spec, (2, nt, nl) if 0 < nt * nl <= (1 << 20) else None, (), stats)


def run_compute_array_taps(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                           rx_elements, tx_elements, array_frequency=None, stats=None):
    """hrt_compute_array_taps through ctypes -> complex64 [nrx, ntx, Nr, Nt, 2, num_times, num_taps] (array_frequency
    defaults to the carrier).  Raises RuntimeError("hrt_compute_array_taps failed (<rc>): ...") on an error code."""
    nr, nt, extra = _array_args(rx_elements, tx_elements, f_ghz, array_frequency)
    # (an output too large for the host is refused by the library's limits first: allocate only what passes them)
    ntm, nl = int(spec.num_times), int(spec.num_taps)
    pts = nr * nt * ntm * nl
    fits = 0 < pts <= (1 << 24) and ntm * nl <= (1 << 20)
    return _run_pathsum(lib, "hrt_compute_array_taps", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths,
                        num_bounces, spec, (nr, nt, 2, ntm, nl) if fits else None, extra, stats)


def run_compute_beam_taps(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                          rx_elements, tx_elements, rx_weights, tx_weights, array_frequency=None, stats=None):
    """hrt_compute_beam_taps through ctypes -> complex64 [nrx, ntx, Br, Bt, 2, num_times, num_taps]: rx_weights
    (Br, Nr) is applied conjugated (the combiner w^H), tx_weights (Bt, Nt) as it is; array_frequency defaults to the
    carrier.  Raises RuntimeError("hrt_compute_beam_taps failed (<rc>): ...") on an error code."""
    nr, nt, extra = _array_args(rx_elements, tx_elements, f_ghz, array_frequency)
    wr, wt = weights(rx_weights, nr, "rx_weights"), weights(tx_weights, nt, "tx_weights")
    br, bt = wr.shape[0], wt.shape[0]
    extra += (wr.ctypes.data_as(c_float_p), C.c_size_t(br), wt.ctypes.data_as(c_float_p), C.c_size_t(bt))
    # (an output too large for the host is refused by the library's limits first: allocate only what passes them)
    ntm, nl = int(spec.num_times), int(spec.num_taps)
    fits = 0 < br * bt * ntm * nl <= (1 << 24) and ntm * nl <= (1 << 20)
    return _run_pathsum(lib, "hrt_compute_beam_taps", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths,
                        num_bounces, spec, (br, bt, 2, ntm, nl) if fits else None, extra, stats)


class PropagateSpec(C.Structure):
    """include/hermespy_rt.h hrt_propagate_spec"""
    _fields_ = [("num_rx", C.c_uint32), ("num_tx", C.c_uint32), ("nr", C.c_uint32), ("nt", C.c_uint32),
                ("num_times", C.c_uint32), ("num_taps", C.c_uint32), ("l_min", C.c_int32),
                ("samples_per_block", C.c_uint32), ("num_samples", C.c_uint64), ("num_out", C.c_uint64)]


def propagate_spec(num_rx, num_tx, nr, nt, num_times, num_taps, l_min, samples_per_block, num_samples, num_out):
    return PropagateSpec(int(num_rx), int(num_tx), int(nr), int(nt), int(num_times), int(num_taps), int(l_min),
                         int(samples_per_block), int(num_samples), int(num_out))


def run_propagate(lib, device, spec, d_taps, d_signal, d_out, accumulate=0, stream=None):
    """hrt_propagate through ctypes on device pointers (integers or None).  Raises RuntimeError("hrt_propagate failed
    (<rc>): ...") on an error code."""
    rc = lib.hrt_propagate(int(device), C.byref(spec) if spec is not None else None, C.c_void_p(d_taps),
                           C.c_void_p(d_signal), C.c_void_p(d_out), int(accumulate), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("hrt_propagate failed (%d): %s" % (rc, lib.hrt_last_error().decode()))


def run_compute_received_signal(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                                rx_elements, tx_elements, signal, samples_per_block=None, num_out=None,
                                array_frequency=None, stats=None):
    """hrt_compute_received_signal through ctypes -> complex64 [nrx, Nr, 2, num_out]: `signal` complex [ntx, Nt, N]
    (or [ntx, N] with Nt = 1; None: a NULL pointer), samples_per_block None: one block of num_out samples; num_out
    defaults to N + L - 1 + max(l_min, 0); array_frequency to the carrier.  Raises
    RuntimeError("hrt_compute_received_signal failed (<rc>): ...") on an error code."""
    nr, nt, extra = _array_args(rx_elements, tx_elements, f_ghz, array_frequency)
    nrx = np.asarray(rx_pos).size // 3
    x, n = None, 0
    if signal is not None:
        x = np.ascontiguousarray(signal, np.complex64)
        n = x.shape[-1] if x.ndim else 0
    if num_out is None:
        num_out = n + int(spec.num_taps) - 1 + max(int(spec.l_min), 0)
    s = max(int(num_out), 1) if samples_per_block is None else int(samples_per_block)
    extra += (C.c_uint32(s), x.ctypes.data_as(c_float_p) if x is not None else None, C.c_uint64(n),
              C.c_uint64(int(num_out)))
    # (an output too large for the host is refused by the library's limits first: allocate only what passes them)
    fits = 0 < nr <= 1024 and 0 < int(num_out) <= 1 << 31
    out = _run_pathsum(lib, "hrt_compute_received_signal", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz,
                       num_paths, num_bounces, spec, (nrx * nr * 2 * int(num_out) * 2,) if fits else None, extra,
                       stats, np.float32)
    if not fits:
        raise RuntimeError("hrt_compute_received_signal accepted a call beyond its limits")
    return out.view(np.complex64).reshape(nrx, nr, 2, int(num_out))


SVD_U, SVD_V = 1, 2              # hrt_svd_spec.want
SVD_NOT_CONVERGED = 0xFFFFFFFF    # a point's `sweeps` at the cap
SVD_MAX_SHORT, SVD_MAX_LONG = 16, 64


class SvdSpec(C.Structure):
    """include/hermespy_rt.h hrt_svd_spec"""
    _fields_ = [("num_rx", C.c_uint32), ("num_tx", C.c_uint32), ("nr", C.c_uint32), ("nt", C.c_uint32),
                ("num_times", C.c_uint32), ("num_freqs", C.c_uint32), ("want", C.c_uint32)]


def svd_spec(num_rx, num_tx, nr, nt, num_times, num_freqs, vectors=True, want=None):
    if want is None:
        want = (SVD_U | SVD_V) if vectors else 0
    return SvdSpec(int(num_rx), int(num_tx), int(nr), int(nt), int(num_times), int(num_freqs), int(want))


def svd_regions(spec):
    """the byte offsets of sigma, u, v, sweeps and the end of an SVD output (hrt_svd_out_bytes is the last)"""
    pts = int(spec.num_rx) * int(spec.num_tx) * 2 * int(spec.num_times) * int(spec.num_freqs)
    nr, nt = int(spec.nr), int(spec.nt)
    n = min(nr, nt)
    o1 = pts * n * 4
    o2 = o1 + (pts * nr * n * 8 if int(spec.want) & SVD_U else 0)
    o3 = o2 + (pts * nt * n * 8 if int(spec.want) & SVD_V else 0)
    return 0, o1, o2, o3, o3 + pts * 4


def svd_views(buf, spec):
    """the regions of a flat uint8 SVD buffer (numpy array or torch tensor) as views: sigma float32 [nrx, ntx, n, 2, T,
    K], u complex64 [nrx, ntx, Nr, n, 2, T, K], v complex64 [nrx, ntx, Nt, n, 2, T, K] (None where not asked for),
    sweeps [nrx, ntx, 2, T, K] (uint32 in numpy; int32 in torch, where SVD_NOT_CONVERGED reads -1), buffer"""
    o = svd_regions(spec)
    nrx, ntx, nr, nt = int(spec.num_rx), int(spec.num_tx), int(spec.nr), int(spec.nt)
    T, K, n = int(spec.num_times), int(spec.num_freqs), min(nr, nt)
    if isinstance(buf, np.ndarray):
        f32, c64, u32 = np.float32, np.complex64, np.uint32
    else:
        import torch
        f32, c64, u32 = torch.float32, torch.complex64, torch.int32
    out = {"sigma": buf[o[0]:o[1]].view(f32).reshape(nrx, ntx, n, 2, T, K), "u": None, "v": None,
           "sweeps": buf[o[3]:o[4]].view(u32).reshape(nrx, ntx, 2, T, K), "buffer": buf}
    if int(spec.want) & SVD_U:
        out["u"] = buf[o[1]:o[2]].view(c64).reshape(nrx, ntx, nr, n, 2, T, K)
    if int(spec.want) & SVD_V:
        out["v"] = buf[o[2]:o[3]].view(c64).reshape(nrx, ntx, nt, n, 2, T, K)
    return out


def run_channel_svd(lib, device, spec, d_H, d_out, stream=None):
    """hrt_channel_svd through ctypes on device pointers (integers or None).  Raises RuntimeError("hrt_channel_svd
    failed (<rc>): ...") on an error code."""
    rc = lib.hrt_channel_svd(int(device), C.byref(spec) if spec is not None else None, C.c_void_p(d_H),
                             C.c_void_p(d_out), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("hrt_channel_svd failed (%d): %s" % (rc, lib.hrt_last_error().decode()))


def run_compute_channel_svd(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                            rx_elements, tx_elements, vectors=True, want=None, array_frequency=None, stats=None):
    """hrt_compute_channel_svd through ctypes -> svd_views of a uint8 numpy buffer (spec: a ChannelSpec, as for
    run_compute_array_channel; array_frequency defaults to the carrier).  Raises
    RuntimeError("hrt_compute_channel_svd failed (<rc>): ...") on an error code."""
    nr, nt, extra = _array_args(rx_elements, tx_elements, f_ghz, array_frequency)
    nrx, ntx = np.asarray(rx_pos).size // 3, np.asarray(tx_pos).size // 3
    sv = svd_spec(nrx, ntx, nr, nt, int(spec.num_times), int(spec.num_freqs), vectors, want)
    extra += (C.c_uint32(int(sv.want)),)
    # (an output too large for the host is refused by the library's limits first: allocate only what passes them)
    grid = int(spec.num_times) * int(spec.num_freqs)
    fits = (0 < min(nr, nt) <= SVD_MAX_SHORT and max(nr, nt) <= SVD_MAX_LONG and 0 < nr * nt * grid <= 1 << 24
            and 0 < nrx * ntx * 2 * grid < 1 << 31 and not int(sv.want) & ~(SVD_U | SVD_V))
    out = _run_pathsum(lib, "hrt_compute_channel_svd", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths,
                       num_bounces, spec, (svd_regions(sv)[4],) if fits else None, extra, stats, np.uint8)
    if not fits:
        raise RuntimeError("hrt_compute_channel_svd accepted a call beyond its limits")
    return svd_views(out, sv)


EQ_ZF, EQ_LMMSE = 0, 1                 # hrt_equalizer_spec.kind
EQ_W = 1                               # hrt_equalizer_spec.flags
EQ_SINGULAR, EQ_NONFINITE = 1, 2       # a point's `status`
EQ_MAX_NT, EQ_MAX_NR = 16, 64
EQ_KINDS = {"zf": EQ_ZF, "lmmse": EQ_LMMSE}


class EqualizerSpec(C.Structure):
    """include/hermespy_rt.h hrt_equalizer_spec"""
    _fields_ = [("num_rx", C.c_uint32), ("num_tx", C.c_uint32), ("nr", C.c_uint32), ("nt", C.c_uint32),
                ("num_times", C.c_uint32), ("num_freqs", C.c_uint32), ("kind", C.c_uint32), ("flags", C.c_uint32),
                ("noise", C.c_float)]


def equalizer_kind(kind):
    """"zf" / "lmmse" (any case) or the constant itself -> hrt_equalizer_spec.kind; an unknown name raises ValueError,
    an unknown number is passed on for the library to refuse"""
    if isinstance(kind, str):
        if kind.lower() not in EQ_KINDS:
            raise ValueError("kind must be 'zf' or 'lmmse', got %r" % (kind,))
        return EQ_KINDS[kind.lower()]
    return int(kind)


def equalizer_spec(num_rx, num_tx, nr, nt, num_times, num_freqs, noise, kind=EQ_LMMSE, weights=True, flags=None):
    if flags is None:
        flags = EQ_W if weights else 0
    return EqualizerSpec(int(num_rx), int(num_tx), int(nr), int(nt), int(num_times), int(num_freqs),
                         equalizer_kind(kind), int(flags), float(noise))


def equalizer_regions(spec):
    """the byte offsets of W, sinr, status and the end of an equalizer output (hrt_equalizer_out_bytes is the last)"""
    pts = int(spec.num_rx) * int(spec.num_tx) * 2 * int(spec.num_times) * int(spec.num_freqs)
    nr, nt = int(spec.nr), int(spec.nt)
    o1 = pts * nt * nr * 8 if int(spec.flags) & EQ_W else 0
    o2 = o1 + pts * nt * 4
    return 0, o1, o2, o2 + pts * 4


def equalizer_views(buf, spec):
    """the regions of a flat uint8 equalizer buffer (numpy array or torch tensor) as views: W complex64 [nrx, ntx, Nt,
    Nr, 2, T, K] (None where not asked for), sinr float32 [nrx, ntx, Nt, 2, T, K], status [nrx, ntx, 2, T, K] (uint32
    in numpy, int32 in torch), buffer"""
    o = equalizer_regions(spec)
    nrx, ntx, nr, nt = int(spec.num_rx), int(spec.num_tx), int(spec.nr), int(spec.nt)
    T, K = int(spec.num_times), int(spec.num_freqs)
    if isinstance(buf, np.ndarray):
        f32, c64, u32 = np.float32, np.complex64, np.uint32
    else:
        import torch
        f32, c64, u32 = torch.float32, torch.complex64, torch.int32
    out = {"W": None, "sinr": buf[o[1]:o[2]].view(f32).reshape(nrx, ntx, nt, 2, T, K),
           "status": buf[o[2]:o[3]].view(u32).reshape(nrx, ntx, 2, T, K), "buffer": buf}
    if int(spec.flags) & EQ_W:
        out["W"] = buf[o[0]:o[1]].view(c64).reshape(nrx, ntx, nt, nr, 2, T, K)
    return out


def run_channel_equalizer(lib, device, spec, d_H, d_out, stream=None):
    """hrt_channel_equalizer through ctypes on device pointers (integers or None).  Raises
    RuntimeError("hrt_channel_equalizer failed (<rc>): ...") on an error code."""
    rc = lib.hrt_channel_equalizer(int(device), C.byref(spec) if spec is not None else None, C.c_void_p(d_H),
                                   C.c_void_p(d_out), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("hrt_channel_equalizer failed (%d): %s" % (rc, lib.hrt_last_error().decode()))


def run_compute_channel_equalizer(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                                  rx_elements, tx_elements, noise, kind=EQ_LMMSE, weights=True, flags=None,
                                  array_frequency=None, stats=None):
    """hrt_compute_channel_equalizer through ctypes -> equalizer_views of a uint8 numpy buffer (spec: a ChannelSpec, as
    for run_compute_array_channel; array_frequency defaults to the carrier).  The equalizer is formed once, of the H
    accumulated over all batches: it is not additive.  Raises RuntimeError("hrt_compute_channel_equalizer failed
    (<rc>): ...") on an error code."""
    nr, nt, extra = _array_args(rx_elements, tx_elements, f_ghz, array_frequency)
    nrx, ntx = np.asarray(rx_pos).size // 3, np.asarray(tx_pos).size // 3
    eq = equalizer_spec(nrx, ntx, nr, nt, int(spec.num_times), int(spec.num_freqs), noise, kind, weights, flags)
    extra += (C.c_uint32(int(eq.kind)), C.c_uint32(int(eq.flags)), C.c_float(float(noise)))
    # (an output too large for the host is refused by the library's limits first: allocate only what passes them)
    grid = int(spec.num_times) * int(spec.num_freqs)
    fits = (0 < nt <= EQ_MAX_NT and 0 < nr <= EQ_MAX_NR and 0 < nr * nt * grid <= 1 << 24
            and 0 < nrx * ntx * 2 * grid < 1 << 31 and not int(eq.flags) & ~EQ_W and int(eq.kind) in (EQ_ZF, EQ_LMMSE)
            and (int(eq.kind) == EQ_LMMSE or nr >= nt) and 0.0 < float(eq.noise) < float("inf"))
    out = _run_pathsum(lib, "hrt_compute_channel_equalizer", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz,
                       num_paths, num_bounces, spec, (equalizer_regions(eq)[3],) if fits else None, extra, stats, np.uint8)
    if not fits:
        raise RuntimeError("hrt_compute_channel_equalizer accepted a call beyond its limits")
    return equalizer_views(out, eq)


PC_MRT, PC_ZF, PC_RZF = 0, 1, 2        # hrt_precoder_spec.kind
PC_TOTAL, PC_STREAM = 0, 1             # hrt_precoder_spec.norm
PC_P = 1                               # hrt_precoder_spec.flags
PC_SINGULAR, PC_NONFINITE = 1, 2       # a point's `status`
PC_MAX_NR, PC_MAX_NT = 16, 64
PC_KINDS = {"mrt": PC_MRT, "zf": PC_ZF, "rzf": PC_RZF}
PC_NORMS = {"total": PC_TOTAL, "stream": PC_STREAM}


class PrecoderSpec(C.Structure):
    """include/hermespy_rt.h hrt_precoder_spec"""
    _fields_ = [("num_rx", C.c_uint32), ("num_tx", C.c_uint32), ("nr", C.c_uint32), ("nt", C.c_uint32),
                ("num_times", C.c_uint32), ("num_freqs", C.c_uint32), ("kind", C.c_uint32), ("norm", C.c_uint32),
                ("flags", C.c_uint32), ("noise", C.c_float), ("power", C.c_float), ("regularization", C.c_float)]


def _pc_name(value, names, what):
    if isinstance(value, str):
        if value.lower() not in names:
            raise ValueError("%s must be one of %s, got %r" % (what, ", ".join(repr(n) for n in names), value))
        return names[value.lower()]
    return int(value)


def precoder_kind(kind):
    """"mrt" / "zf" / "rzf" (any case) or the constant itself -> hrt_precoder_spec.kind; an unknown name raises
    ValueError, an unknown number is passed on for the library to refuse"""
    return _pc_name(kind, PC_KINDS, "kind")


def precoder_norm(norm):
    """"total" / "stream" (any case) or the constant itself -> hrt_precoder_spec.norm, as precoder_kind"""
    return _pc_name(norm, PC_NORMS, "normalize")


def precoder_spec(num_rx, num_tx, nr, nt, num_times, num_freqs, noise, kind=PC_RZF, power=1.0, regularization=None,
                  normalize=PC_TOTAL, weights=True, flags=None):
    """regularization None: Nr N0 / Ptot under RZF (precode.default_regularization), 0 (not read) otherwise"""
    if flags is None:
        flags = PC_P if weights else 0
    kind = precoder_kind(kind)
    if regularization is None:
        ok = kind == PC_RZF and float(power) > 0.0
        regularization = int(nr) * float(noise) / float(power) if ok else 0.0
    return PrecoderSpec(int(num_rx), int(num_tx), int(nr), int(nt), int(num_times), int(num_freqs), kind,
                        precoder_norm(normalize), int(flags), float(noise), float(power), float(regularization))


def precoder_regions(spec):
    """the byte offsets of P, sinr, status and the end of a precoder output (hrt_precoder_out_bytes is the last)"""
    pts = int(spec.num_rx) * int(spec.num_tx) * 2 * int(spec.num_times) * int(spec.num_freqs)
    nr, nt = int(spec.nr), int(spec.nt)
    o1 = pts * nt * nr * 8 if int(spec.flags) & PC_P else 0
    o2 = o1 + pts * nr * 4
    return 0, o1, o2, o2 + pts * 4


def precoder_views(buf, spec):
    """the regions of a flat uint8 precoder buffer (numpy array or torch tensor) as views: P complex64 [nrx, ntx, Nt,
    Nr, 2, T, K] (None where not asked for), sinr float32 [nrx, ntx, Nr, 2, T, K], status [nrx, ntx, 2, T, K] (uint32
    in numpy, int32 in torch), buffer"""
    o = precoder_regions(spec)
    nrx, ntx, nr, nt = int(spec.num_rx), int(spec.num_tx), int(spec.nr), int(spec.nt)
    T, K = int(spec.num_times), int(spec.num_freqs)
    if isinstance(buf, np.ndarray):
        f32, c64, u32 = np.float32, np.complex64, np.uint32
    else:
        import torch
        f32, c64, u32 = torch.float32, torch.complex64, torch.int32
    out = {"P": None, "sinr": buf[o[1]:o[2]].view(f32).reshape(nrx, ntx, nr, 2, T, K),
           "status": buf[o[2]:o[3]].view(u32).reshape(nrx, ntx, 2, T, K), "buffer": buf}
    if int(spec.flags) & PC_P:
        out["P"] = buf[o[0]:o[1]].view(c64).reshape(nrx, ntx, nt, nr, 2, T, K)
    return out


def _pc_positive(v):
    return 0.0 < float(v) < float("inf")


def precoder_fits(spec):
    """whether the library accepts the spec (its limits, mirrored: an output beyond them is not allocated)"""
    grid = int(spec.num_times) * int(spec.num_freqs)
    nr, nt, kind = int(spec.nr), int(spec.nt), int(spec.kind)
    return (0 < nr <= PC_MAX_NR and 0 < nt <= PC_MAX_NT and 0 < nr * nt * grid <= 1 << 24
            and 0 < int(spec.num_rx) * int(spec.num_tx) * 2 * grid < 1 << 31 and not int(spec.flags) & ~PC_P
            and kind in (PC_MRT, PC_ZF, PC_RZF) and int(spec.norm) in (PC_TOTAL, PC_STREAM)
            and (kind != PC_ZF or nr <= nt) and _pc_positive(spec.noise) and _pc_positive(spec.power)
            and (kind != PC_RZF or _pc_positive(spec.regularization)))


def run_channel_precoder(lib, device, spec, d_H, d_out, stream=None):
    """hrt_channel_precoder through ctypes on device pointers (integers or None).  Raises
    RuntimeError("hrt_channel_precoder failed (<rc>): ...") on an error code."""
    rc = lib.hrt_channel_precoder(int(device), C.byref(spec) if spec is not None else None, C.c_void_p(d_H),
                                  C.c_void_p(d_out), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("hrt_channel_precoder failed (%d): %s" % (rc, lib.hrt_last_error().decode()))


def run_compute_channel_precoder(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                                 rx_elements, tx_elements, noise, kind=PC_RZF, power=1.0, regularization=None,
                                 normalize=PC_TOTAL, weights=True, flags=None, array_frequency=None, stats=None):
    """hrt_compute_channel_precoder through ctypes -> precoder_views of a uint8 numpy buffer (spec: a ChannelSpec, as
    for run_compute_array_channel; array_frequency defaults to the carrier).  The precoder is formed once, of the H
    accumulated over all batches: it is not additive.  Raises RuntimeError("hrt_compute_channel_precoder failed
    (<rc>): ...") on an error code."""
    nr, nt, extra = _array_args(rx_elements, tx_elements, f_ghz, array_frequency)
    nrx, ntx = np.asarray(rx_pos).size // 3, np.asarray(tx_pos).size // 3
    pc = precoder_spec(nrx, ntx, nr, nt, int(spec.num_times), int(spec.num_freqs), noise, kind, power, regularization,
                       normalize, weights, flags)
    extra += (C.c_uint32(int(pc.kind)), C.c_uint32(int(pc.norm)), C.c_uint32(int(pc.flags)), C.c_float(pc.noise),
              C.c_float(pc.power), C.c_float(pc.regularization))
    fits = precoder_fits(pc)
    out = _run_pathsum(lib, "hrt_compute_channel_precoder", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz,
                       num_paths, num_bounces, spec, (precoder_regions(pc)[3],) if fits else None, extra, stats, np.uint8)
    if not fits:
        raise RuntimeError("hrt_compute_channel_precoder accepted a call beyond its limits")
    return precoder_views(out, pc)


CS_POWER, CS_CAPACITY = 0, 1           # hrt_codebook_spec.metric
CS_TABLE, CS_EFFECTIVE = 1, 2          # hrt_codebook_spec.flags
CS_NONFINITE = 1                       # a subband's `status`
CS_NO_INDEX = 0xFFFFFFFF               # a flagged subband's `index`
CS_MAX_NR, CS_MAX_NT, CS_MAX_L, CS_MAX_C = 16, 64, 4, 4096
CS_METRICS = {"power": CS_POWER, "capacity": CS_CAPACITY}


class CodebookSpec(C.Structure):
    """include/hermespy_rt.h hrt_codebook_spec"""
    _fields_ = [("num_rx", C.c_uint32), ("num_tx", C.c_uint32), ("nr", C.c_uint32), ("nt", C.c_uint32),
                ("num_times", C.c_uint32), ("num_freqs", C.c_uint32), ("layers", C.c_uint32), ("entries", C.c_uint32),
                ("subband", C.c_uint32), ("metric", C.c_uint32), ("flags", C.c_uint32), ("noise", C.c_float)]


def codebook_metric(metric):
    """"power" / "capacity" (any case) or the constant itself -> hrt_codebook_spec.metric; an unknown name raises
    ValueError, an unknown number is passed on for the library to refuse"""
    return _pc_name(metric, CS_METRICS, "metric")


def codebook_spec(num_rx, num_tx, nr, nt, num_times, num_freqs, layers, entries, metric=CS_CAPACITY, noise=None,
                  subband=None, table=False, effective=False, flags=None):
    """subband None: wideband (S = K); noise None: 1.0 under POWER (not read), refused under CAPACITY (0)"""
    if flags is None:
        flags = (CS_TABLE if table else 0) | (CS_EFFECTIVE if effective else 0)
    metric = codebook_metric(metric)
    if noise is None:
        noise = 1.0 if metric == CS_POWER else 0.0
    return CodebookSpec(int(num_rx), int(num_tx), int(nr), int(nt), int(num_times), int(num_freqs), int(layers),
                        int(entries), int(num_freqs) if subband is None else int(subband), metric, int(flags),
                        float(noise))


def codebook_subbands(spec):
    """B = ceil(K / S) (0 where S is 0)"""
    S = int(spec.subband)
    return (int(spec.num_freqs) + S - 1) // S if S > 0 else 0


def codebook_regions(spec):
    """the byte offsets of index, metric, status, table, effective and the end of a codebook selection output
    (hrt_codebook_out_bytes is the last)"""
    links = int(spec.num_rx) * int(spec.num_tx)
    sub = links * 2 * int(spec.num_times) * codebook_subbands(spec)
    pts = links * 2 * int(spec.num_times) * int(spec.num_freqs)
    o3 = 3 * sub * 4
    o4 = o3 + (sub * int(spec.entries) * 4 if int(spec.flags) & CS_TABLE else 0)
    o5 = o4 + (pts * int(spec.nr) * int(spec.layers) * 8 if int(spec.flags) & CS_EFFECTIVE else 0)
    return 0, sub * 4, 2 * sub * 4, o3, o4, o5


def codebook_views(buf, spec):
    """the regions of a flat uint8 codebook selection buffer (numpy array or torch tensor) as views: index [nrx, ntx, 2,
    T, B] (uint32 in numpy, int32 in torch: a flagged subband reads -1 there), metric float32 and status of that shape,
    table float32 [nrx, ntx, C, 2, T, B] and effective complex64 [nrx, ntx, Nr, L, 2, T, K] (None where not asked
    for), buffer"""
    o = codebook_regions(spec)
    nrx, ntx, nr = int(spec.num_rx), int(spec.num_tx), int(spec.nr)
    T, K, B = int(spec.num_times), int(spec.num_freqs), codebook_subbands(spec)
    if isinstance(buf, np.ndarray):
        f32, c64, u32 = np.float32, np.complex64, np.uint32
    else:
        import torch
        f32, c64, u32 = torch.float32, torch.complex64, torch.int32
    out = {"index": buf[o[0]:o[1]].view(u32).reshape(nrx, ntx, 2, T, B),
           "metric": buf[o[1]:o[2]].view(f32).reshape(nrx, ntx, 2, T, B),
           "status": buf[o[2]:o[3]].view(u32).reshape(nrx, ntx, 2, T, B), "table": None, "effective": None,
           "buffer": buf}
    if int(spec.flags) & CS_TABLE:
        out["table"] = buf[o[3]:o[4]].view(f32).reshape(nrx, ntx, int(spec.entries), 2, T, B)
    if int(spec.flags) & CS_EFFECTIVE:
        out["effective"] = buf[o[4]:o[5]].view(c64).reshape(nrx, ntx, nr, int(spec.layers), 2, T, K)
    return out


def codebook_fits(spec):
    """whether the library accepts the spec (its limits, mirrored: an output beyond them is not allocated)"""
    grid = int(spec.num_times) * int(spec.num_freqs)
    nr, nt, L, Cn, S = int(spec.nr), int(spec.nt), int(spec.layers), int(spec.entries), int(spec.subband)
    links = int(spec.num_rx) * int(spec.num_tx)
    return (0 < nr <= CS_MAX_NR and 0 < nt <= CS_MAX_NT and 0 < L <= min(CS_MAX_L, nt) and 0 < Cn <= CS_MAX_C
            and 0 < S <= int(spec.num_freqs) and 0 < links * 2 * grid < 1 << 31
            and links * 2 * int(spec.num_times) * codebook_subbands(spec) * Cn < 1 << 31
            and int(spec.metric) in (CS_POWER, CS_CAPACITY) and not int(spec.flags) & ~(CS_TABLE | CS_EFFECTIVE)
            and (int(spec.metric) == CS_POWER or _pc_positive(spec.noise)))


def codebook_array(codebook, nt=None):
    """a codebook as a contiguous complex64 [C, Nt, L] numpy array ([C, Nt] is taken as L = 1)"""
    a = np.asarray(codebook)
    if a.dtype.kind not in "fc":
        raise ValueError("codebook must be a real or complex floating-point array, got %s" % (a.dtype,))
    a = np.ascontiguousarray(a, np.complex64)
    if a.ndim == 2:
        a = a.reshape(a.shape[0], a.shape[1], 1)
    if a.ndim != 3 or (nt is not None and a.shape[1] != nt):
        raise ValueError("codebook must have shape (C, %s, L), got %s" % ("Nt" if nt is None else nt, a.shape))
    return a


def run_codebook_select(lib, device, spec, d_H, d_codebook, d_out, stream=None):
    """hrt_codebook_select through ctypes on device pointers (integers or None).  Raises
    RuntimeError("hrt_codebook_select failed (<rc>): ...") on an error code."""
    rc = lib.hrt_codebook_select(int(device), C.byref(spec) if spec is not None else None, C.c_void_p(d_H),
                                 C.c_void_p(d_codebook), C.c_void_p(d_out), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("hrt_codebook_select failed (%d): %s" % (rc, lib.hrt_last_error().decode()))


def run_compute_codebook_select(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                                rx_elements, tx_elements, codebook, metric=CS_CAPACITY, noise=None, subband=None,
                                table=False, effective=False, flags=None, array_frequency=None, stats=None):
    """hrt_compute_codebook_select through ctypes -> codebook_views of a uint8 numpy buffer (spec: a ChannelSpec, as
    for run_compute_array_channel; codebook: complex [C, Nt, L], None passes NULL; array_frequency defaults to the
    carrier).  The selection runs once, on the H accumulated over all batches: it is not additive.  Raises
    RuntimeError("hrt_compute_codebook_select failed (<rc>): ...") on an error code."""
    nr, nt, extra = _array_args(rx_elements, tx_elements, f_ghz, array_frequency)
    nrx, ntx = np.asarray(rx_pos).size // 3, np.asarray(tx_pos).size // 3
    if codebook is None:
        cb, entries, layers = None, 1, 1
    else:
        cb = codebook_array(codebook)
        entries, layers = cb.shape[0], cb.shape[2]
    cs = codebook_spec(nrx, ntx, nr, nt, int(spec.num_times), int(spec.num_freqs), layers, entries, metric, noise,
                       subband, table, effective, flags)
    extra += (cb.ctypes.data_as(C.POINTER(C.c_float)) if cb is not None else None, C.c_uint32(layers),
              C.c_uint32(entries), C.c_uint32(int(cs.subband)), C.c_uint32(int(cs.metric)), C.c_uint32(int(cs.flags)),
              C.c_float(cs.noise))
    fits = codebook_fits(cs) and cb is not None and cb.shape[1] == nt
    out = _run_pathsum(lib, "hrt_compute_codebook_select", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz,
                       num_paths, num_bounces, spec, (codebook_regions(cs)[5],) if fits else None, extra, stats, np.uint8)
    if not fits:
        raise RuntimeError("hrt_compute_codebook_select accepted a call beyond its limits")
    return codebook_views(out, cs)


DT_LLR = 1                             # hrt_detect_spec.flags
DT_NONFINITE = 1                       # a point's `status`
DT_NO_INDEX = 0xFFFFFFFF               # a flagged point's `index`
DT_MAX_NR, DT_MAX_B, DT_MAX_BITS = 64, 8, 12


class DetectSpec(C.Structure):
    """include/hermespy_rt.h hrt_detect_spec"""
    _fields_ = [("num_rx", C.c_uint32), ("num_tx", C.c_uint32), ("nr", C.c_uint32), ("nt", C.c_uint32),
                ("num_times", C.c_uint32), ("num_freqs", C.c_uint32), ("bits", C.c_uint32), ("flags", C.c_uint32),
                ("noise", C.c_float)]


def detect_spec(num_rx, num_tx, nr, nt, num_times, num_freqs, bits, noise, llr=True, flags=None):
    if flags is None:
        flags = DT_LLR if llr else 0
    return DetectSpec(int(num_rx), int(num_tx), int(nr), int(nt), int(num_times), int(num_freqs), int(bits),
                      int(flags), float(noise))


def detect_regions(spec):
    """the byte offsets of index, metric, status, llr and the end of a detection output (hrt_detect_out_bytes is the
    last)"""
    pts = int(spec.num_rx) * int(spec.num_tx) * 2 * int(spec.num_times) * int(spec.num_freqs)
    o3 = 3 * pts * 4
    return 0, pts * 4, 2 * pts * 4, o3, o3 + (pts * int(spec.nt) * int(spec.bits) * 4 if int(spec.flags) & DT_LLR else 0)


def detect_views(buf, spec):
    """the regions of a flat uint8 detection buffer (numpy array or torch tensor) as views: index [nrx, ntx, 2, T, K]
    (uint32 in numpy, int32 in torch: a flagged point reads -1 there), metric float32 and status of that shape, llr
    float32 [nrx, ntx, Nt, B, 2, T, K] (None where not asked for), buffer"""
    o = detect_regions(spec)
    nrx, ntx, T, K = int(spec.num_rx), int(spec.num_tx), int(spec.num_times), int(spec.num_freqs)
    if isinstance(buf, np.ndarray):
        f32, u32 = np.float32, np.uint32
    else:
        import torch
        f32, u32 = torch.float32, torch.int32
    out = {"index": buf[o[0]:o[1]].view(u32).reshape(nrx, ntx, 2, T, K),
           "metric": buf[o[1]:o[2]].view(f32).reshape(nrx, ntx, 2, T, K),
           "status": buf[o[2]:o[3]].view(u32).reshape(nrx, ntx, 2, T, K), "llr": None, "buffer": buf}
    if int(spec.flags) & DT_LLR:
        out["llr"] = buf[o[3]:o[4]].view(f32).reshape(nrx, ntx, int(spec.nt), int(spec.bits), 2, T, K)
    return out


def detect_fits(spec):
    """whether the library accepts the spec (its limits, mirrored: an output beyond them is not allocated)"""
    grid = int(spec.num_times) * int(spec.num_freqs)
    nr, nt, b = int(spec.nr), int(spec.nt), int(spec.bits)
    return (0 < nr <= DT_MAX_NR and 0 < b <= DT_MAX_B and 0 < nt and nt * b <= DT_MAX_BITS
            and 0 < nr * nt * grid <= 1 << 24 and 0 < int(spec.num_rx) * int(spec.num_tx) * 2 * grid < 1 << 31
            and not int(spec.flags) & ~DT_LLR and _pc_positive(spec.noise))


def constellation_array(constellation):
    """a constellation as a contiguous complex64 [M] numpy array and its B (M = 2^B; -1 where M is no power of two)"""
    a = np.asarray(constellation)
    if a.dtype.kind not in "fc":
        raise ValueError("constellation must be a real or complex floating-point array, got %s" % (a.dtype,))
    a = np.ascontiguousarray(a, np.complex64)
    if a.ndim != 1:
        raise ValueError("constellation must have shape (M,), got %s" % (a.shape,))
    m = a.shape[0]
    return a, (m.bit_length() - 1 if m >= 2 and not m & (m - 1) else -1)


def run_channel_detect(lib, device, spec, d_H, d_Y, d_constellation, d_out, stream=None):
    """hrt_channel_detect through ctypes on device pointers (integers or None).  Raises
    RuntimeError("hrt_channel_detect failed (<rc>): ...") on an error code."""
    rc = lib.hrt_channel_detect(int(device), C.byref(spec) if spec is not None else None, C.c_void_p(d_H),
                                C.c_void_p(d_Y), C.c_void_p(d_constellation), C.c_void_p(d_out), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("hrt_channel_detect failed (%d): %s" % (rc, lib.hrt_last_error().decode()))


def run_compute_channel_detect(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                               rx_elements, tx_elements, Y, constellation, noise, llr=True, flags=None,
                               array_frequency=None, stats=None):
    """hrt_compute_channel_detect through ctypes -> detect_views of a uint8 numpy buffer (spec: a ChannelSpec, as for
    run_compute_array_channel; Y: complex [nrx, ntx, Nr, 2, T, K] and constellation: complex [2^B], None passes NULL;
    array_frequency defaults to the carrier).  Detection runs once, on the H accumulated over all batches: it is not
    additive.  A Y of another shape or a constellation whose size is no power of two raises ValueError (the library
    cannot see either).  Raises RuntimeError("hrt_compute_channel_detect failed (<rc>): ...") on an error code."""
    nr, nt, extra = _array_args(rx_elements, tx_elements, f_ghz, array_frequency)
    nrx, ntx = np.asarray(rx_pos).size // 3, np.asarray(tx_pos).size // 3
    fp = C.POINTER(C.c_float)
    if constellation is None:
        s, b = None, 1
    else:
        s, b = constellation_array(constellation)
        if b < 0:
            raise ValueError("constellation must hold 2^B symbols, got %d" % s.shape[0])
    ds = detect_spec(nrx, ntx, nr, nt, int(spec.num_times), int(spec.num_freqs), b, noise, llr, flags)
    y = None if Y is None else np.ascontiguousarray(Y, np.complex64)
    if y is not None and y.shape != (nrx, ntx, nr, 2, int(spec.num_times), int(spec.num_freqs)):
        raise ValueError("Y [%d, %d, %d, 2, %d, %d] expected, got %s"
                         % (nrx, ntx, nr, int(spec.num_times), int(spec.num_freqs), y.shape))
    extra += (y.ctypes.data_as(fp) if y is not None else None, s.ctypes.data_as(fp) if s is not None else None,
              C.c_uint32(int(ds.bits)), C.c_uint32(int(ds.flags)), C.c_float(ds.noise))
    fits = detect_fits(ds) and s is not None and y is not None
    out = _run_pathsum(lib, "hrt_compute_channel_detect", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz,
                       num_paths, num_bounces, spec, (detect_regions(ds)[4],) if fits else None, extra, stats, np.uint8)
    if not fits:
        raise RuntimeError("hrt_compute_channel_detect accepted a call beyond its limits")
    return detect_views(out, ds)


KB_LLR, KB_SORTED = 1, 2               # hrt_kbest_spec.flags
KB_NONFINITE, KB_DEFICIENT = 1, 2       # a point's `status`
KB_NO_INDEX = 0xFFFFFFFF                # a non-finite point's `index` (status decides: with Nt B = 32 it is a hypothesis)
KB_MAX_NR, KB_MAX_NT, KB_MAX_B, KB_MAX_BITS, KB_MAX_K = 64, 16, 8, 32, 64


class KbestSpec(C.Structure):
    """include/hermespy_rt.h hrt_kbest_spec"""
    _fields_ = [("num_rx", C.c_uint32), ("num_tx", C.c_uint32), ("nr", C.c_uint32), ("nt", C.c_uint32),
                ("num_times", C.c_uint32), ("num_freqs", C.c_uint32), ("bits", C.c_uint32), ("flags", C.c_uint32),
                ("k", C.c_uint32), ("noise", C.c_float), ("clip", C.c_float)]


def kbest_spec(num_rx, num_tx, nr, nt, num_times, num_freqs, bits, noise, k, clip, sorted=True, llr=True,
               flags=None):
    if flags is None:
        flags = (KB_LLR if llr else 0) | (KB_SORTED if sorted else 0)
    return KbestSpec(int(num_rx), int(num_tx), int(nr), int(nt), int(num_times), int(num_freqs), int(bits),
                     int(flags), int(k), float(noise), float(clip))


def kbest_regions(spec):
    """the byte offsets of index, metric, status, llr and the end of a K-best detection output (hrt_kbest_out_bytes
    is the last): detect_regions' layout"""
    pts = int(spec.num_rx) * int(spec.num_tx) * 2 * int(spec.num_times) * int(spec.num_freqs)
    o3 = 3 * pts * 4
    return 0, pts * 4, 2 * pts * 4, o3, o3 + (pts * int(spec.nt) * int(spec.bits) * 4 if int(spec.flags) & KB_LLR else 0)


def kbest_views(buf, spec):
    """the regions of a flat uint8 K-best detection buffer as views, as detect_views gives them: index, metric, status
    [nrx, ntx, 2, T, K], llr float32 [nrx, ntx, Nt, B, 2, T, K] (None where not asked for), buffer"""
    o = kbest_regions(spec)
    nrx, ntx, T, K = int(spec.num_rx), int(spec.num_tx), int(spec.num_times), int(spec.num_freqs)
    if isinstance(buf, np.ndarray):
        f32, u32 = np.float32, np.uint32
    else:
        import torch
        f32, u32 = torch.float32, torch.int32
    out = {"index": buf[o[0]:o[1]].view(u32).reshape(nrx, ntx, 2, T, K),
           "metric": buf[o[1]:o[2]].view(f32).reshape(nrx, ntx, 2, T, K),
           "status": buf[o[2]:o[3]].view(u32).reshape(nrx, ntx, 2, T, K), "llr": None, "buffer": buf}
    if int(spec.flags) & KB_LLR:
        out["llr"] = buf[o[3]:o[4]].view(f32).reshape(nrx, ntx, int(spec.nt), int(spec.bits), 2, T, K)
    return out


def kbest_fits(spec):
    """whether the library accepts the spec (its limits, mirrored: an output beyond them is not allocated)"""
    grid = int(spec.num_times) * int(spec.num_freqs)
    nr, nt, b, k = int(spec.nr), int(spec.nt), int(spec.bits), int(spec.k)
    return (0 < nr <= KB_MAX_NR and 0 < b <= KB_MAX_B and 0 < nt <= KB_MAX_NT and nt * b <= KB_MAX_BITS
            and 0 < k <= KB_MAX_K and not k & (k - 1)
            and 0 < nr * nt * grid <= 1 << 24 and 0 < int(spec.num_rx) * int(spec.num_tx) * 2 * grid < 1 << 31
            and not int(spec.flags) & ~(KB_LLR | KB_SORTED) and _pc_positive(spec.noise) and _pc_positive(spec.clip))


def run_kbest(lib, device, spec, d_H, d_Y, d_constellation, d_out, stream=None):
    """hrt_channel_kbest through ctypes on device pointers (integers or None).  Raises
    RuntimeError("hrt_channel_kbest failed (<rc>): ...") on an error code."""
    rc = lib.hrt_channel_kbest(int(device), C.byref(spec) if spec is not None else None, C.c_void_p(d_H),
                               C.c_void_p(d_Y), C.c_void_p(d_constellation), C.c_void_p(d_out), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("hrt_channel_kbest failed (%d): %s" % (rc, lib.hrt_last_error().decode()))


def run_compute_channel_kbest(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                              rx_elements, tx_elements, Y, constellation, noise, k, clip, sorted=True, llr=True,
                              flags=None, array_frequency=None, stats=None):
    """hrt_compute_channel_kbest through ctypes -> kbest_views of a uint8 numpy buffer; the arguments are
    run_compute_channel_detect's, with the list size k, the LLR clip and the ordering switch.  Detection runs once,
    on the H accumulated over all batches.  A Y of another shape or a constellation whose size is no power of two
    raises ValueError.  Raises RuntimeError("hrt_compute_channel_kbest failed (<rc>): ...") on an error code."""
    nr, nt, extra = _array_args(rx_elements, tx_elements, f_ghz, array_frequency)
    nrx, ntx = np.asarray(rx_pos).size // 3, np.asarray(tx_pos).size // 3
    fp = C.POINTER(C.c_float)
    if constellation is None:
        s, b = None, 1
    else:
        s, b = constellation_array(constellation)
        if b < 0:
            raise ValueError("constellation must hold 2^B symbols, got %d" % s.shape[0])
    ks = kbest_spec(nrx, ntx, nr, nt, int(spec.num_times), int(spec.num_freqs), b, noise, k, clip, sorted, llr, flags)
    y = None if Y is None else np.ascontiguousarray(Y, np.complex64)
    if y is not None and y.shape != (nrx, ntx, nr, 2, int(spec.num_times), int(spec.num_freqs)):
        raise ValueError("Y [%d, %d, %d, 2, %d, %d] expected, got %s"
                         % (nrx, ntx, nr, int(spec.num_times), int(spec.num_freqs), y.shape))
    extra += (y.ctypes.data_as(fp) if y is not None else None, s.ctypes.data_as(fp) if s is not None else None,
              C.c_uint32(int(ks.bits)), C.c_uint32(int(ks.flags)), C.c_uint32(int(ks.k)), C.c_float(ks.noise),
              C.c_float(ks.clip))
    fits = kbest_fits(ks) and s is not None and y is not None
    out = _run_pathsum(lib, "hrt_compute_channel_kbest", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz,
                       num_paths, num_bounces, spec, (kbest_regions(ks)[4],) if fits else None, extra, stats, np.uint8)
    if not fits:
        raise RuntimeError("hrt_compute_channel_kbest accepted a call beyond its limits")
    return kbest_views(out, ks)


# hrt_power_spec: the moments' field indices (include/hermespy_rt.h HRT_POWER_*)
(POWER_COUNT, POWER_P, POWER_P_TAU, POWER_P_TAU2, POWER_P_NU, POWER_P_NU2, POWER_P_URX_X, POWER_P_URX_Y,
 POWER_P_URX_Z, POWER_P_UTX_X, POWER_P_UTX_Y, POWER_P_UTX_Z, POWER_P_LOS, POWER_FIELDS) = range(14)


class PowerSpec(C.Structure):
    """include/hermespy_rt.h hrt_power_spec"""
    _fields_ = [("tau0_s", C.c_double), ("dtau_s", C.c_double), ("num_delay_bins", C.c_uint32),
                ("num_zenith_bins", C.c_uint32), ("num_azimuth_bins", C.c_uint32), ("parts", C.c_uint32)]


def power_spec(tau0, dtau, num_delay_bins, num_zenith_bins=0, num_azimuth_bins=0, los=True, scatter=True,
               parts=None):
    if parts is None:
        parts = (CHANNEL_LOS if los else 0) | (CHANNEL_SCATTER if scatter else 0)
    return PowerSpec(float(tau0), float(dtau), int(num_delay_bins), int(num_zenith_bins), int(num_azimuth_bins),
                     int(parts))


def power_out_doubles(nrx, ntx, spec):
    """the doubles of a power profiles output (hrt_power_out_doubles)"""
    return nrx * ntx * 2 * (POWER_FIELDS + int(spec.num_delay_bins) +
                            2 * int(spec.num_zenith_bins) * int(spec.num_azimuth_bins))


def power_views(buf, nrx, ntx, spec):
    """the regions of a flat power profiles buffer (numpy array or torch tensor) as views: moments [nrx, ntx, 2, F],
    pdp [nrx, ntx, 2, Ld], arrival and departure [nrx, ntx, 2, Nth, Nph] (zero-sized where switched off), buffer"""
    ld, nth, nph = int(spec.num_delay_bins), int(spec.num_zenith_bins), int(spec.num_azimuth_bins)
    lp = nrx * ntx * 2
    o1 = lp * POWER_FIELDS
    o2 = o1 + lp * ld
    o3 = o2 + lp * nth * nph
    o4 = o3 + lp * nth * nph
    return {"moments": buf[:o1].reshape(nrx, ntx, 2, POWER_FIELDS),
            "pdp": buf[o1:o2].reshape(nrx, ntx, 2, ld),
            "arrival": buf[o2:o3].reshape(nrx, ntx, 2, nth, nph),
            "departure": buf[o3:o4].reshape(nrx, ntx, 2, nth, nph),
            "buffer": buf}


def run_compute_power_profiles(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                               stats=None):
    """hrt_compute_power_profiles through ctypes -> power_views of a float64 numpy buffer.  Raises
    RuntimeError("hrt_compute_power_profiles failed (<rc>): ...") on an error code."""
    nrx, ntx = np.asarray(rx_pos).size // 3, np.asarray(tx_pos).size // 3
    # (an output too large for the host is refused by the library's limits first: allocate only what passes them)
    n = power_out_doubles(nrx, ntx, spec)
    out = _run_pathsum(lib, "hrt_compute_power_profiles", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths,
                       num_bounces, spec, (n,) if n <= 2 * (POWER_FIELDS * 65535 + (1 << 26)) else None, (), stats,
                       np.float64)
    return power_views(out, nrx, ntx, spec)


COV_RX, COV_TX = 1, 2       # hrt_covariance_spec.sides
COV_MAX_ELEMENTS = 256      # per side; and num_rx * num_tx * 2 * (Nr^2 + Nt^2) <= 2^26


class CovarianceSpec(C.Structure):
    """include/hermespy_rt.h hrt_covariance_spec"""
    _fields_ = [("parts", C.c_uint32), ("sides", C.c_uint32)]


def covariance_spec(rx=True, tx=True, los=True, scatter=True, parts=None, sides=None):
    if parts is None:
        parts = (CHANNEL_LOS if los else 0) | (CHANNEL_SCATTER if scatter else 0)
    if sides is None:
        sides = (COV_RX if rx else 0) | (COV_TX if tx else 0)
    return CovarianceSpec(int(parts), int(sides))


def covariance_out_floats(nrx, ntx, arrays, spec):
    """the floats of a covariance output (hrt_covariance_out_floats): arrays an ArraySpec, or (Nr, Nt)"""
    nr, nt = (arrays.num_rx_elements, arrays.num_tx_elements) if isinstance(arrays, ArraySpec) else arrays
    nr = int(nr) if int(spec.sides) & COV_RX else 0
    nt = int(nt) if int(spec.sides) & COV_TX else 0
    return nrx * ntx * 2 * (nr * nr + nt * nt) * 2


def covariance_views(buf, nrx, ntx, nr, nt):
    """the regions of a flat complex64 covariance buffer (numpy array or torch tensor) as views: rx [nrx, ntx, 2, Nr,
    Nr], tx [nrx, ntx, 2, Nt, Nt] (nr / nt 0: the side is absent, a zero-sized view), buffer"""
    o1 = nrx * ntx * 2 * nr * nr
    o2 = o1 + nrx * ntx * 2 * nt * nt
    return {"rx": buf[:o1].reshape(nrx, ntx, 2, nr, nr), "tx": buf[o1:o2].reshape(nrx, ntx, 2, nt, nt), "buffer": buf}


def run_compute_array_covariance(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                                 rx_elements=None, tx_elements=None, array_frequency=None, stats=None):
    """hrt_compute_array_covariance through ctypes -> covariance_views of a complex64 numpy buffer (elements None: no
    elements for that side; array_frequency defaults to the carrier).  Raises
    RuntimeError("hrt_compute_array_covariance failed (<rc>): ...") on an error code."""
    none = np.zeros((0, 3), np.float32)
    nr, nt, extra = _array_args(none if rx_elements is None else rx_elements,
                                none if tx_elements is None else tx_elements, f_ghz, array_frequency)
    if rx_elements is None:
        extra = (None,) + extra[1:]
    if tx_elements is None:
        extra = extra[:2] + (None,) + extra[3:]
    nrx, ntx = np.asarray(rx_pos).size // 3, np.asarray(tx_pos).size // 3
    # (an output too large for the host is refused by the library's limits first: allocate only what passes them)
    n = covariance_out_floats(nrx, ntx, (nr, nt), spec)
    fits = nr <= COV_MAX_ELEMENTS and nt <= COV_MAX_ELEMENTS and 0 < n <= 1 << 27 and nrx * ntx <= 65535
    out = _run_pathsum(lib, "hrt_compute_array_covariance", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz,
                       num_paths, num_bounces, spec, (n,) if fits else None, extra, stats, np.float32)
    if not fits:
        raise RuntimeError("hrt_compute_array_covariance accepted a call beyond its limits")
    return covariance_views(out.view(np.complex64), nrx, ntx, nr if int(spec.sides) & COV_RX else 0,
                            nt if int(spec.sides) & COV_TX else 0)


class Pattern(C.Structure):
    """include/hermespy_rt.h hrt_pattern (d_table: a device pointer in PatternSpec, a host pointer in PatternsHost)"""
    _fields_ = [("kind", C.c_uint32), ("num_zenith", C.c_uint32), ("num_azimuth", C.c_uint32),
                ("gain_db", C.c_float), ("d_table", C.c_void_p)]


class PatternSpec(C.Structure):
    """include/hrt_device.h hrt_pattern_spec (device pointers)"""
    _fields_ = [("rx", Pattern), ("tx", Pattern), ("d_rx_rot", C.c_void_p), ("d_tx_rot", C.c_void_p)]


class PatternsHost(C.Structure):
    """include/hermespy_rt.h hrt_patterns_host (host pointers)"""
    _fields_ = [("rx", Pattern), ("tx", Pattern), ("rx_rot", C.c_void_p), ("tx_rot", C.c_void_p),
                ("num_rx", C.c_size_t), ("num_tx", C.c_size_t)]


def pattern_struct(p, table_ptr=None):
    """the hrt_pattern of a pattern dict (hermespy_rt_amd.patterns) whose table is at table_ptr"""
    t = None if p.get("table") is None else np.asarray(p["table"])
    nz, na = (int(t.shape[0]), int(t.shape[1])) if t is not None and t.ndim == 2 else (0, 0)
    return Pattern(int(p["kind"]), nz, na, float(p["gain_db"]), table_ptr)


class compute_patterns:
    """with abi.compute_patterns(lib, rx=..., tx=..., rx_orientation=..., tx_orientation=...): the path-sum drop-in
    calls (run_compute_channel, ...) of this thread inside the block apply the patterns (hrt_compute_set_patterns).
    The patterns are pattern dicts (None: isotropic), the orientations float32 [n, 3, 3] arrays (None: identity); what
    the library refuses is refused by the call inside the block."""

    def __init__(self, lib, rx=None, tx=None, rx_orientation=None, tx_orientation=None):
        from . import patterns as _pt
        self.lib = lib
        rx, tx = _pt.isotropic() if rx is None else rx, _pt.isotropic() if tx is None else tx
        self.keep = []

        def ptr(a):
            if a is None:
                return None, 0
            a = np.ascontiguousarray(np.asarray(a, np.float32))
            self.keep.append(a)
            return a.ctypes.data, a.shape[0]

        rr, nrx = ptr(rx_orientation)
        tr, ntx = ptr(tx_orientation)
        self.host = PatternsHost(pattern_struct(rx, ptr(rx.get("table"))[0]), pattern_struct(tx, ptr(tx.get("table"))[0]),
                                 rr, tr, nrx, ntx)

    def __enter__(self):
        self.lib.hrt_compute_set_patterns(C.byref(self.host))
        return self

    def __exit__(self, *exc):
        self.lib.hrt_compute_set_patterns(None)
        return False


DOMINANT_MAX_PATHS = 1024   # hrt_dominant_spec.max_paths; and num_rx * num_tx * max_paths <= 2^22


class DominantSpec(C.Structure):
    """include/hermespy_rt.h hrt_dominant_spec"""
    _fields_ = [("max_paths", C.c_uint32), ("parts", C.c_uint32)]


class DominantPath(C.Structure):
    """include/hermespy_rt.h hrt_dominant_path"""
    _fields_ = [("power", C.c_double), ("path", C.c_uint64), ("bounce", C.c_int32), ("tri", C.c_uint32),
                ("a_te_re", C.c_float), ("a_te_im", C.c_float), ("a_tm_re", C.c_float), ("a_tm_im", C.c_float),
                ("tau", C.c_float), ("freq_shift", C.c_float), ("u_rx", C.c_float * 3), ("u_tx", C.c_float * 3)]


assert C.sizeof(DominantSpec) == 8 and C.sizeof(DominantPath) == 72


def dominant_spec(max_paths, los=True, scatter=True, parts=None):
    if parts is None:
        parts = (CHANNEL_LOS if los else 0) | (CHANNEL_SCATTER if scatter else 0)
    return DominantSpec(int(max_paths), int(parts))


def dominant_out_bytes(nrx, ntx, spec):
    """the bytes of a dominant paths output (hrt_dominant_out_bytes; 0 for a spec the library refuses)"""
    k, links = int(spec.max_paths), nrx * ntx
    if not 0 < k <= DOMINANT_MAX_PATHS or not int(spec.parts) or int(spec.parts) & ~3:
        return 0
    if max(nrx, ntx, links) > 65535 or links * k > (1 << 22):
        return 0
    return links * (16 + k * C.sizeof(DominantPath))


def dominant_views(buf, nrx, ntx, K):
    """the fields of a dominant paths buffer (a flat uint8 numpy array or torch tensor, 8-byte aligned) as views, no
    copies: kept, eligible [nrx, ntx]; power, path, bounce, tri, tau, freq_shift [nrx, ntx, K]; a_te, a_tm complex64
    [nrx, ntx, K]; u_rx, u_tx [nrx, ntx, K, 3]; buffer"""
    links, K = nrx * ntx, int(K)
    is_np = isinstance(buf, np.ndarray)
    if is_np:
        i32, u32, i64, u64, f32, f64 = np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64
    else:
        import torch
        i32, i64, f32, f64 = torch.int32, torch.int64, torch.float32, torch.float64
        u32, u64 = i32, i64   # (torch: the unsigned fields as their signed bit patterns)
    hdr = buf[:16 * links].view(u64).reshape(nrx, ntx, 2)
    rec = buf[16 * links:16 * links + 72 * links * K]
    w64 = rec.view(i64).reshape(nrx, ntx, K, 9)
    w32 = rec.view(i32).reshape(nrx, ntx, K, 18)

    def cplx(lo):
        pair = w32[..., lo:lo + 2].view(f32)   # [nrx, ntx, K, 2]: re, im next to each other
        if is_np:
            return pair.view(np.complex64)[..., 0]
        return torch.view_as_complex(pair)

    return {"kept": hdr[..., 0], "eligible": hdr[..., 1],
            "power": w64[..., 0].view(f64), "path": w64[..., 1].view(u64),
            "bounce": w32[..., 4], "tri": w32[..., 5].view(u32),
            "a_te": cplx(6), "a_tm": cplx(8),
            "tau": w32[..., 10].view(f32), "freq_shift": w32[..., 11].view(f32),
            "u_rx": w32[..., 12:15].view(f32), "u_tx": w32[..., 15:18].view(f32), "buffer": buf}


def run_compute_dominant_paths(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces, spec,
                               stats=None):
    """hrt_compute_dominant_paths through ctypes -> dominant_views of a uint8 numpy buffer.  Raises
    RuntimeError("hrt_compute_dominant_paths failed (<rc>): ...") on an error code."""
    nrx, ntx = np.asarray(rx_pos).size // 3, np.asarray(tx_pos).size // 3
    # (an output too large for the host is refused by the library's limits first: allocate only what passes them)
    n = dominant_out_bytes(nrx, ntx, spec)
    out = _run_pathsum(lib, "hrt_compute_dominant_paths", scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths,
                       num_bounces, spec, (n,) if n else None, (), stats, np.uint8)
    return dominant_views(out, nrx, ntx, spec.max_paths)


# ---- the array channel of dominant-path lists (include/hermespy_rt.h: hrt_sparse_spec) ----
class SparseSpec(C.Structure):
    """include/hermespy_rt.h hrt_sparse_spec"""
    _fields_ = [("f0_hz", C.c_double), ("df_hz", C.c_double), ("num_freqs", C.c_uint32),
                ("t0_s", C.c_double), ("dt_s", C.c_double), ("num_times", C.c_uint32),
                ("num_rx", C.c_uint32), ("num_tx", C.c_uint32), ("max_paths", C.c_uint32)]


assert C.sizeof(SparseSpec) == 56


def sparse_spec(num_rx, num_tx, max_paths, f0, df, num_freqs, t0=0.0, dt=0.0, num_times=1):
    return SparseSpec(float(f0), float(df), int(num_freqs), float(t0), float(dt), int(num_times), int(num_rx),
                      int(num_tx), int(max_paths))


def sparse_paths_bytes(spec):
    """the bytes of the lists a sparse spec reads (hrt_sparse_paths_bytes; 0 for a spec the library refuses)"""
    links, k = int(spec.num_rx) * int(spec.num_tx), int(spec.max_paths)
    grid = int(spec.num_freqs) * int(spec.num_times)
    if not 0 < links <= 65535 or not 0 < k <= DOMINANT_MAX_PATHS or links * k > (1 << 22):
        return 0
    if not 0 < grid <= (1 << 20) or not all(np.isfinite([spec.f0_hz, spec.df_hz, spec.t0_s, spec.dt_s])):
        return 0
    return links * (16 + k * C.sizeof(DominantPath))


def sparse_out_bytes(spec, nr, nt):
    """the bytes of a sparse array channel (hrt_sparse_out_bytes; 0 for a spec the library refuses)"""
    if not sparse_paths_bytes(spec):
        return 0
    return int(spec.num_rx) * int(spec.num_tx) * int(nr) * int(nt) * 2 * int(spec.num_times) * int(spec.num_freqs) * 8


def run_sparse_array_channel(lib, device, spec, d_rx_el, nr, d_tx_el, nt, fa_hz, d_paths, d_out, accumulate=0,
                             stream=None):
    """hrt_sparse_array_channel through ctypes on device pointers (integers or None).  Raises
    RuntimeError("hrt_sparse_array_channel failed (<rc>): ...") on an error code."""
    rc = lib.hrt_sparse_array_channel(int(device), C.byref(spec) if spec is not None else None, C.c_void_p(d_rx_el),
                                      C.c_uint32(int(nr)), C.c_void_p(d_tx_el), C.c_uint32(int(nt)),
                                      C.c_double(float(fa_hz)), C.c_void_p(d_paths), C.c_void_p(d_out),
                                      C.c_int(int(accumulate)), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("hrt_sparse_array_channel failed (%d): %s" % (rc, lib.hrt_last_error().decode()))


def run_compute_sparse_array_channel(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces,
                                     dominant, grid, rx_elements, tx_elements, array_frequency=None, return_paths=False,
                                     stats=None):
    """hrt_compute_sparse_array_channel through ctypes (dominant: a DominantSpec, grid: a ChannelSpec whose parts are
    not read) -> complex64 [nrx, ntx, Nr, Nt, 2, num_times, num_freqs], or (H, dominant_views of the lists) with
    return_paths.  Raises RuntimeError("hrt_compute_sparse_array_channel failed (<rc>): ...") on an error code."""
    rx_pos = np.asarray(rx_pos, np.float32).reshape(-1, 3)
    tx_pos = np.asarray(tx_pos, np.float32).reshape(-1, 3)
    nrx, ntx = rx_pos.shape[0], tx_pos.shape[0]
    _, rxp = _vec3_arg(rx_pos, nrx)
    _, txp = _vec3_arg(tx_pos, ntx)
    rxv_a, rxv = _vec3_arg(rx_vel, nrx)
    txv_a, txv = _vec3_arg(tx_vel, ntx)
    nr, nt, extra = _array_args(rx_elements, tx_elements, f_ghz, array_frequency)
    # (outputs too large for the host are refused by the library's limits first: allocate only what passes them)
    T, K = (int(grid.num_times), int(grid.num_freqs)) if grid is not None else (0, 0)
    pts = nr * nt * T * K
    nbytes = dominant_out_bytes(nrx, ntx, dominant) if dominant is not None else 0
    fits = nbytes > 0 and 0 < pts <= (1 << 24) and T * K <= (1 << 20)
    out = np.zeros((nrx, ntx, nr, nt, 2, T, K) if fits else (1,), np.complex64)
    paths = np.zeros(nbytes if fits else 8, np.uint8) if return_paths else None
    scene = lib.scene_load(str(scene_path).encode())
    try:
        rc = lib.hrt_compute_sparse_array_channel(
            C.byref(scene), rxp, txp, rxv, txv, C.c_float(f_ghz), C.c_size_t(nrx), C.c_size_t(ntx),
            C.c_size_t(int(num_paths)), C.c_size_t(int(num_bounces)),
            C.byref(dominant) if dominant is not None else None, C.byref(grid) if grid is not None else None, *extra,
            out.ctypes.data_as(c_float_p), paths.ctypes.data_as(C.c_void_p) if paths is not None else None,
            C.byref(stats) if stats is not None else None)
    finally:
        free_scene(scene)
    if rc != 0:
        raise RuntimeError("hrt_compute_sparse_array_channel failed (%d): %s" % (rc, lib.hrt_last_error().decode()))
    if not fits:
        raise RuntimeError("hrt_compute_sparse_array_channel accepted a call beyond its limits")
    return (out, dominant_views(paths, nrx, ntx, dominant.max_paths)) if return_paths else out


# ---- the beam channel of dominant-path lists (include/hermespy_rt.h: hrt_compute_sparse_beam_channel) ----
def sparse_beam_out_bytes(spec, br, bt):
    """the bytes of the beam channel of a list (hrt_sparse_beam_out_bytes; 0 for a spec the library refuses)"""
    if not sparse_paths_bytes(spec):
        return 0
    return int(spec.num_rx) * int(spec.num_tx) * int(br) * int(bt) * 2 * int(spec.num_times) * int(spec.num_freqs) * 8


def run_sparse_beam_channel(lib, device, spec, d_rx_el, nr, d_tx_el, nt, fa_hz, d_rx_w, br, d_tx_w, bt, d_paths, d_out,
                            accumulate=0, stream=None):
    """hrt_sparse_beam_channel through ctypes on device pointers (integers or None).  Raises
    RuntimeError("hrt_sparse_beam_channel failed (<rc>): ...") on an error code."""
    rc = lib.hrt_sparse_beam_channel(int(device), C.byref(spec) if spec is not None else None, C.c_void_p(d_rx_el),
                                     C.c_uint32(int(nr)), C.c_void_p(d_tx_el), C.c_uint32(int(nt)),
                                     C.c_double(float(fa_hz)), C.c_void_p(d_rx_w), C.c_uint32(int(br)),
                                     C.c_void_p(d_tx_w), C.c_uint32(int(bt)), C.c_void_p(d_paths), C.c_void_p(d_out),
                                     C.c_int(int(accumulate)), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("hrt_sparse_beam_channel failed (%d): %s" % (rc, lib.hrt_last_error().decode()))


def run_compute_sparse_beam_channel(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces,
                                    dominant, grid, rx_elements, tx_elements, rx_weights, tx_weights,
                                    array_frequency=None, return_paths=False, stats=None):
    """hrt_compute_sparse_beam_channel through ctypes (dominant: a DominantSpec, grid: a ChannelSpec whose parts are
    not read) -> complex64 [nrx, ntx, Br, Bt, 2, num_times, num_freqs], or (B, dominant_views of the lists) with
    return_paths.  rx_weights (Br, Nr) is applied conjugated, tx_weights (Bt, Nt) as it is.  Raises
    RuntimeError("hrt_compute_sparse_beam_channel failed (<rc>): ...") on an error code."""
    rx_pos = np.asarray(rx_pos, np.float32).reshape(-1, 3)
    tx_pos = np.asarray(tx_pos, np.float32).reshape(-1, 3)
    nrx, ntx = rx_pos.shape[0], tx_pos.shape[0]
    _, rxp = _vec3_arg(rx_pos, nrx)
    _, txp = _vec3_arg(tx_pos, ntx)
    rxv_a, rxv = _vec3_arg(rx_vel, nrx)
    txv_a, txv = _vec3_arg(tx_vel, ntx)
    nr, nt, extra = _array_args(rx_elements, tx_elements, f_ghz, array_frequency)
    wr, wt = weights(rx_weights, nr, "rx_weights"), weights(tx_weights, nt, "tx_weights")
    br, bt = wr.shape[0], wt.shape[0]
    extra += (wr.ctypes.data_as(c_float_p), C.c_size_t(br), wt.ctypes.data_as(c_float_p), C.c_size_t(bt))
    # (outputs too large for the host are refused by the library's limits first: allocate only what passes them)
    T, K = (int(grid.num_times), int(grid.num_freqs)) if grid is not None else (0, 0)
    pts = br * bt * T * K
    nbytes = dominant_out_bytes(nrx, ntx, dominant) if dominant is not None else 0
    fits = nbytes > 0 and 0 < pts <= (1 << 24) and T * K <= (1 << 20)
    out = np.zeros((nrx, ntx, br, bt, 2, T, K) if fits else (1,), np.complex64)
    paths = np.zeros(nbytes if fits else 8, np.uint8) if return_paths else None
    scene = lib.scene_load(str(scene_path).encode())
    try:
        rc = lib.hrt_compute_sparse_beam_channel(
            C.byref(scene), rxp, txp, rxv, txv, C.c_float(f_ghz), C.c_size_t(nrx), C.c_size_t(ntx),
            C.c_size_t(int(num_paths)), C.c_size_t(int(num_bounces)),
            C.byref(dominant) if dominant is not None else None, C.byref(grid) if grid is not None else None, *extra,
            out.ctypes.data_as(c_float_p), paths.ctypes.data_as(C.c_void_p) if paths is not None else None,
            C.byref(stats) if stats is not None else None)
    finally:
        free_scene(scene)
    if rc != 0:
        raise RuntimeError("hrt_compute_sparse_beam_channel failed (%d): %s" % (rc, lib.hrt_last_error().decode()))
    if not fits:
        raise RuntimeError("hrt_compute_sparse_beam_channel accepted a call beyond its limits")
    return (out, dominant_views(paths, nrx, ntx, dominant.max_paths)) if return_paths else out


# ---- the array taps of dominant-path lists (include/hermespy_rt.h: hrt_sparse_taps_spec) ----
class SparseTapsSpec(C.Structure):
    """include/hermespy_rt.h hrt_sparse_taps_spec"""
    _fields_ = [("fs_hz", C.c_double), ("fc_hz", C.c_double), ("t0_s", C.c_double), ("dt_s", C.c_double),
                ("l_min", C.c_int32), ("num_taps", C.c_uint32), ("num_times", C.c_uint32),
                ("num_rx", C.c_uint32), ("num_tx", C.c_uint32), ("max_paths", C.c_uint32)]


assert C.sizeof(SparseTapsSpec) == 56


def sparse_taps_spec(num_rx, num_tx, max_paths, fs, num_taps, l_min=0, fc=0.0, t0=0.0, dt=0.0, num_times=1):
    return SparseTapsSpec(float(fs), float(fc), float(t0), float(dt), int(l_min), int(num_taps), int(num_times),
                          int(num_rx), int(num_tx), int(max_paths))


def sparse_taps_out_bytes(spec, nr, nt):
    """the bytes of the array taps of a list (hrt_sparse_taps_out_bytes; 0 for a spec the library refuses)"""
    links, k = int(spec.num_rx) * int(spec.num_tx), int(spec.max_paths)
    L, T, lo = int(spec.num_taps), int(spec.num_times), int(spec.l_min)
    if not 0 < links <= 65535 or not 0 < k <= DOMINANT_MAX_PATHS or links * k > (1 << 22):
        return 0
    if L == 0 or T == 0 or L * T > (1 << 20) or abs(lo) > (1 << 24) or lo + L > (1 << 24):
        return 0
    if not all(np.isfinite([spec.fs_hz, spec.fc_hz, spec.t0_s, spec.dt_s])) or not spec.fs_hz > 0.0:
        return 0
    return links * int(nr) * int(nt) * 2 * T * L * 8


def run_sparse_array_taps(lib, device, spec, d_rx_el, nr, d_tx_el, nt, fa_hz, d_paths, d_out, accumulate=0,
                          stream=None):
    """hrt_sparse_array_taps through ctypes on device pointers (integers or None).  Raises
    RuntimeError("hrt_sparse_array_taps failed (<rc>): ...") on an error code."""
    rc = lib.hrt_sparse_array_taps(int(device), C.byref(spec) if spec is not None else None, C.c_void_p(d_rx_el),
                                   C.c_uint32(int(nr)), C.c_void_p(d_tx_el), C.c_uint32(int(nt)),
                                   C.c_double(float(fa_hz)), C.c_void_p(d_paths), C.c_void_p(d_out),
                                   C.c_int(int(accumulate)), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("hrt_sparse_array_taps failed (%d): %s" % (rc, lib.hrt_last_error().decode()))


def run_compute_sparse_array_taps(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces,
                                  dominant, grid, rx_elements, tx_elements, array_frequency=None, return_paths=False,
                                  stats=None):
    """hrt_compute_sparse_array_taps through ctypes (dominant: a DominantSpec, grid: a TapsSpec whose parts are not
    read) -> complex64 [nrx, ntx, Nr, Nt, 2, num_times, num_taps], or (h, dominant_views of the lists) with
    return_paths.  Raises RuntimeError("hrt_compute_sparse_array_taps failed (<rc>): ...") on an error code."""
    rx_pos = np.asarray(rx_pos, np.float32).reshape(-1, 3)
    tx_pos = np.asarray(tx_pos, np.float32).reshape(-1, 3)
    nrx, ntx = rx_pos.shape[0], tx_pos.shape[0]
    _, rxp = _vec3_arg(rx_pos, nrx)
    _, txp = _vec3_arg(tx_pos, ntx)
    rxv_a, rxv = _vec3_arg(rx_vel, nrx)
    txv_a, txv = _vec3_arg(tx_vel, ntx)
    nr, nt, extra = _array_args(rx_elements, tx_elements, f_ghz, array_frequency)
    # (outputs too large for the host are refused by the library's limits first: allocate only what passes them)
    T, L = (int(grid.num_times), int(grid.num_taps)) if grid is not None else (0, 0)
    pts = nr * nt * T * L
    nbytes = dominant_out_bytes(nrx, ntx, dominant) if dominant is not None else 0
    fits = nbytes > 0 and 0 < pts <= (1 << 24) and T * L <= (1 << 20)
    out = np.zeros((nrx, ntx, nr, nt, 2, T, L) if fits else (1,), np.complex64)
    paths = np.zeros(nbytes if fits else 8, np.uint8) if return_paths else None
    scene = lib.scene_load(str(scene_path).encode())
    try:
        rc = lib.hrt_compute_sparse_array_taps(
            C.byref(scene), rxp, txp, rxv, txv, C.c_float(f_ghz), C.c_size_t(nrx), C.c_size_t(ntx),
            C.c_size_t(int(num_paths)), C.c_size_t(int(num_bounces)),
            C.byref(dominant) if dominant is not None else None, C.byref(grid) if grid is not None else None, *extra,
            out.ctypes.data_as(c_float_p), paths.ctypes.data_as(C.c_void_p) if paths is not None else None,
            C.byref(stats) if stats is not None else None)
    finally:
        free_scene(scene)
    if rc != 0:
        raise RuntimeError("hrt_compute_sparse_array_taps failed (%d): %s" % (rc, lib.hrt_last_error().decode()))
    if not fits:
        raise RuntimeError("hrt_compute_sparse_array_taps accepted a call beyond its limits")
    return (out, dominant_views(paths, nrx, ntx, dominant.max_paths)) if return_paths else out


# ---- the beam taps of dominant-path lists (include/hermespy_rt.h: hrt_compute_sparse_beam_taps) ----
def sparse_beam_taps_out_bytes(spec, br, bt):
    """the bytes of the beam taps of a list (hrt_sparse_beam_taps_out_bytes; 0 for a spec the library refuses)"""
    if not sparse_taps_out_bytes(spec, 1, 1):
        return 0
    return int(spec.num_rx) * int(spec.num_tx) * int(br) * int(bt) * 2 * int(spec.num_times) * int(spec.num_taps) * 8


def run_sparse_beam_taps(lib, device, spec, d_rx_el, nr, d_tx_el, nt, fa_hz, d_rx_w, br, d_tx_w, bt, d_paths, d_out,
                         accumulate=0, stream=None):
    """hrt_sparse_beam_taps through ctypes on device pointers (integers or None).  Raises
    RuntimeError("hrt_sparse_beam_taps failed (<rc>): ...") on an error code."""
    rc = lib.hrt_sparse_beam_taps(int(device), C.byref(spec) if spec is not None else None, C.c_void_p(d_rx_el),
                                  C.c_uint32(int(nr)), C.c_void_p(d_tx_el), C.c_uint32(int(nt)),
                                  C.c_double(float(fa_hz)), C.c_void_p(d_rx_w), C.c_uint32(int(br)),
                                  C.c_void_p(d_tx_w), C.c_uint32(int(bt)), C.c_void_p(d_paths), C.c_void_p(d_out),
                                  C.c_int(int(accumulate)), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("hrt_sparse_beam_taps failed (%d): %s" % (rc, lib.hrt_last_error().decode()))


def run_compute_sparse_beam_taps(lib, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces,
                                 dominant, grid, rx_elements, tx_elements, rx_weights, tx_weights,
                                 array_frequency=None, return_paths=False, stats=None):
    """hrt_compute_sparse_beam_taps through ctypes (dominant: a DominantSpec, grid: a TapsSpec whose parts are not read)
    -> complex64 [nrx, ntx, Br, Bt, 2, num_times, num_taps], or (h, dominant_views of the lists) with return_paths.
    rx_weights (Br, Nr) is applied conjugated, tx_weights (Bt, Nt) as it is.  Raises
    RuntimeError("hrt_compute_sparse_beam_taps failed (<rc>): ...") on an error code."""
    rx_pos = np.asarray(rx_pos, np.float32).reshape(-1, 3)
    tx_pos = np.asarray(tx_pos, np.float32).reshape(-1, 3)
    nrx, ntx = rx_pos.shape[0], tx_pos.shape[0]
    _, rxp = _vec3_arg(rx_pos, nrx)
    _, txp = _vec3_arg(tx_pos, ntx)
    rxv_a, rxv = _vec3_arg(rx_vel, nrx)
    txv_a, txv = _vec3_arg(tx_vel, ntx)
    nr, nt, extra = _array_args(rx_elements, tx_elements, f_ghz, array_frequency)
    wr, wt = weights(rx_weights, nr, "rx_weights"), weights(tx_weights, nt, "tx_weights")
    br, bt = wr.shape[0], wt.shape[0]
    extra += (wr.ctypes.data_as(c_float_p), C.c_size_t(br), wt.ctypes.data_as(c_float_p), C.c_size_t(bt))
    # (outputs too large for the host are refused by the library's limits first: allocate only what passes them)
    T, L = (int(grid.num_times), int(grid.num_taps)) if grid is not None else (0, 0)
    pts = br * bt * T * L
    nbytes = dominant_out_bytes(nrx, ntx, dominant) if dominant is not None else 0
    fits = nbytes > 0 and 0 < pts <= (1 << 24) and T * L <= (1 << 20)
    out = np.zeros((nrx, ntx, br, bt, 2, T, L) if fits else (1,), np.complex64)
    paths = np.zeros(nbytes if fits else 8, np.uint8) if return_paths else None
    scene = lib.scene_load(str(scene_path).encode())
    try:
        rc = lib.hrt_compute_sparse_beam_taps(
            C.byref(scene), rxp, txp, rxv, txv, C.c_float(f_ghz), C.c_size_t(nrx), C.c_size_t(ntx),
            C.c_size_t(int(num_paths)), C.c_size_t(int(num_bounces)),
            C.byref(dominant) if dominant is not None else None, C.byref(grid) if grid is not None else None, *extra,
            out.ctypes.data_as(c_float_p), paths.ctypes.data_as(C.c_void_p) if paths is not None else None,
            C.byref(stats) if stats is not None else None)
    finally:
        free_scene(scene)
    if rc != 0:
        raise RuntimeError("hrt_compute_sparse_beam_taps failed (%d): %s" % (rc, lib.hrt_last_error().decode()))
    if not fits:
        raise RuntimeError("hrt_compute_sparse_beam_taps accepted a call beyond its limits")
    return (out, dominant_views(paths, nrx, ntx, dominant.max_paths)) if return_paths else out


# ---- test-only entries (include/hrt_device.h): a lane's own candidate lookup, what the tables were built with ----
CAND_KINDS = dict(patch=1, image=2, txcell=4, cell_mask=8)


def debug_candidates(lib, problem, mode, queries):
    """hrt_debug_candidates: queries float32 [n][8] (o, d, row and apex as u32 bits) -> uint32 [n][10] (served, patch
    index, eight mask words).  Raises RuntimeError on an error code (e.g. no table for the mode)."""
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 8)
    out = np.zeros((q.shape[0], 10), np.uint32)
    rc = lib.hrt_debug_candidates(problem, int(mode), q.shape[0], q.ctypes.data_as(c_float_p),
                                  out.ctypes.data_as(C.POINTER(C.c_uint32)))
    if rc != 0:
        raise RuntimeError("hrt_debug_candidates failed (%d): %s" % (rc, lib.hrt_last_error().decode()))
    return out


def debug_table_info(lib, problem):
    """hrt_debug_table_info -> dict(nuv uint32 [T][2], hmax, ro_rx, ro_img, num_patch, kinds)."""
    T = int(lib.hrt_problem_num_triangles(problem))
    nuv = np.zeros((max(T, 1), 2), np.uint32)
    f3 = np.zeros(3, np.float32)
    npatch, kinds = C.c_uint64(0), C.c_uint32(0)
    rc = lib.hrt_debug_table_info(problem, nuv.ctypes.data_as(C.POINTER(C.c_uint32)), f3.ctypes.data_as(c_float_p),
                                  C.byref(npatch), C.byref(kinds))
    if rc != 0:
        raise RuntimeError("hrt_debug_table_info failed (%d): %s" % (rc, lib.hrt_last_error().decode()))
    return dict(nuv=nuv[:T], hmax=f3[0], ro_rx=f3[1], ro_img=f3[2], num_patch=int(npatch.value), kinds=int(kinds.value))


def debug_last_launch(lib, problem, shard, workspace_ptr, workspace_bytes):
    """hrt_debug_last_launch: launch nb = shard.num_bounces alone (shadow traces + scatter records of bounce nb - 1) on
    the live list the caller planted in the workspace (hit block nb - 1, counts[nb]).  Blocks until done.  Raises
    RuntimeError on an error code (a refusal launches nothing)."""
    rc = lib.hrt_debug_last_launch(problem, C.byref(shard), C.c_void_p(int(workspace_ptr)), C.c_uint64(int(workspace_bytes)))
    if rc != 0:
        raise RuntimeError("hrt_debug_last_launch failed (%d): %s" % (rc, lib.hrt_last_error().decode()))
