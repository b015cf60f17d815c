"""Device-resident tracer: the hot path on torch-owned HBM buffers and streams.

torch is plumbing here (device memory, streams, torch.distributed); the work is done by
hrt_trace() of libhermespy_rt_amd.so on the CURRENT torch stream, called through the C ABI
with raw device pointers.

    tr = Tracer(scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths, num_bounces,
                rank=0, world=1)
    tr.trace()                 # asynchronous on torch's current stream
    counts = tr.counts()       # [nb+2] numpy (syncs)
    hits = tr.hits(b)          # dict name -> torch view of the first H_b elements
    recs = tr.records(b)       # dict name -> [nrx, H_b] torch views, + 'unblocked' bool
"""
import ctypes as C

import numpy as np

from . import abi
from . import lib as _lib


class Tracer:
    def __init__(self, scene_path, rx_pos, tx_pos, rx_vel, tx_vel, f_ghz, num_paths,
                 num_bounces, rank=0, world=1, chunk=0, device=None, host_threads=0, coherent=True,
                 device_dirs=False):
        import torch  # torch first: its HIP runtime is the one the library binds to

        if not torch.cuda.is_available():
            raise _lib.HrtError("no HIP device visible to torch; hermespy-rt_amd has no CPU path")
        self.torch = torch
        self.L = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        rx_pos = np.ascontiguousarray(np.asarray(rx_pos, np.float32).reshape(-1, 3))
        tx_pos = np.ascontiguousarray(np.asarray(tx_pos, np.float32).reshape(-1, 3))
        self.nrx, self.ntx = rx_pos.shape[0], tx_pos.shape[0]
        rx_vel = np.ascontiguousarray(np.asarray(rx_vel, np.float32).reshape(self.nrx, 3))
        tx_vel = np.ascontiguousarray(np.asarray(tx_vel, np.float32).reshape(self.ntx, 3))
        self.num_paths, self.nb = int(num_paths), int(num_bounces)
        self.f_ghz = float(f_ghz)
        V3 = C.POINTER(abi.Vec3)

        scene = self.L.scene_load(str(scene_path).encode())
        try:
            h = C.c_void_p()
            _lib.check(self.L.hrt_problem_create(
                C.byref(scene), rx_pos.ctypes.data_as(V3), tx_pos.ctypes.data_as(V3),
                rx_vel.ctypes.data_as(V3), tx_vel.ctypes.data_as(V3), C.c_float(self.f_ghz),
                self.nrx, self.ntx, self.device.index, C.byref(h)), "hrt_problem_create")
            self.problem = h
        finally:
            abi.free_scene(scene)
        self.num_tri = int(self.L.hrt_problem_num_triangles(self.problem))
        # rows of the device table are in a spatial order (acceleration structure); tri_order[row]
        # = the flat index the reference's (mesh, face) scan gives that triangle
        self.tri_order = np.empty(max(self.num_tri, 1), np.uint32)
        _lib.check(self.L.hrt_problem_tri_order(self.problem,
                                                self.tri_order.ctypes.data_as(C.POINTER(C.c_uint32))),
                   "hrt_problem_tri_order")

        self.shard = _lib.Shard(self.num_paths, rank, world, chunk, self.nb)
        self.num_local = int(self.L.hrt_shard_num_local(C.byref(self.shard)))
        self.layout = _lib.Layout()
        _lib.check(self.L.hrt_layout_query(self.problem, C.byref(self.shard), C.byref(self.layout)),
                   "hrt_layout_query")
        self.cap = int(self.layout.cap)

        # launch directions of this shard, once: host libm (bit-identical to the reference by
        # construction), or generated on the device with the host patching the few values whose
        # float rounding could depend on the math library (bit-identical too; see hrt_device.h)
        self.dirs_patched = None
        if device_dirs:
            with torch.cuda.device(self.device):
                self.dirs = torch.empty((self.num_local, 3), dtype=torch.float32, device=self.device)
            n_p = C.c_uint64(0)
            _lib.check(self.L.hrt_launch_dirs_device(
                C.byref(self.shard), C.c_void_p(self.dirs.data_ptr()), self.device.index,
                C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), C.byref(n_p)),
                "hrt_launch_dirs_device")
            self.dirs_patched = int(n_p.value)
            dirs = None
        else:
            dirs = np.empty((self.num_local, 3), np.float32)
            _lib.check(self.L.hrt_launch_dirs_host(
                C.byref(self.shard), dirs.ctypes.data_as(C.POINTER(C.c_float)), host_threads),
                "hrt_launch_dirs_host")
        self.dirs_host = dirs
        # coherent launch order: a wave = a narrow ray packet (speed only; results are keyed
        # by ray id)
        self.order_host = None
        order_dev = None
        if coherent and device_dirs:
            # ... and the coherent order on the device too (hrt_launch_order_device)
            with torch.cuda.device(self.device):
                order_dev = torch.empty(self.num_local, dtype=torch.int32, device=self.device)
            _lib.check(self.L.hrt_launch_order_device(
                C.byref(self.shard), C.c_void_p(order_dev.data_ptr()), self.device.index,
                C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "hrt_launch_order_device")
        elif coherent:
            order = np.empty(self.num_local, np.uint32)
            _lib.check(self.L.hrt_launch_order_host(
                C.byref(self.shard), dirs.ctypes.data_as(C.POINTER(C.c_float)) if dirs is not None else None,
                order.ctypes.data_as(C.POINTER(C.c_uint32))), "hrt_launch_order_host")
            self.order_host = order
        with torch.cuda.device(self.device):
            if dirs is not None:
                self.dirs = torch.from_numpy(dirs).to(self.device)
            self.order = order_dev if order_dev is not None else (
                torch.from_numpy(self.order_host.view(np.int32)).to(self.device) if coherent else None)
            # the launch set is traced again and again: permute the direction table into launch
            # order ONCE, so the launch kernels read contiguous runs (HRT_DIRS_IN_LAUNCH_ORDER)
            self.flags = 0
            if coherent:
                self.dirs_launch = self.dirs[self.order.to(torch.int64) & 0xFFFFFFFF].contiguous()
                self.flags = _lib.DIRS_IN_LAUNCH_ORDER
            self.ws = torch.empty(int(self.layout.total_bytes), dtype=torch.uint8, device=self.device)
        assert self.ws.data_ptr() % 256 == 0
        self.last_times = None
        self._patterns = None      # (abi.PatternSpec, the device tensor it points into) while patterns are set
        self.patterned = False     # the workspace's amplitudes are weighted by the patterns (since the last trace)

    def close(self):
        if getattr(self, "problem", None):
            self.L.hrt_problem_destroy(self.problem)
            self.problem = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ run
    def trace(self, timed=False):
        """Enqueue the whole path on torch's current stream.  timed=True records HIP events
        around every launch on that stream, waits, and returns (los_ms, [trace_ms per launch]);
        shade / compaction times are in last_shade_ms / last_compact_ms."""
        torch = self.torch
        stream = torch.cuda.current_stream(self.device).cuda_stream
        times = _lib.KernelTimes() if timed else None
        if timed:
            t = self.new_timer()
            self.trace_with_timer(t)
            _lib.check(self.L.hrt_timer_read(t, C.byref(times)), "hrt_timer_read")
            self.L.hrt_timer_destroy(t)
        else:
            _lib.check(self.L.hrt_trace_flags(
                self.problem, C.byref(self.shard), C.c_void_p(self._dirs_ptr()),
                C.c_void_p(self.order.data_ptr()) if self.order is not None else None,
                C.c_void_p(self.ws.data_ptr()), C.c_uint64(self.ws.numel()), C.c_void_p(stream),
                None, C.c_uint32(self.flags)), "hrt_trace_flags")
            self._after_trace()
        if timed:
            n = int(times.num_bounce_launches)
            self.last_times = (float(times.los_ms), [float(times.trace_ms[i]) for i in range(n)])
            self.last_shade_ms = [float(times.shade_ms[i]) for i in range(n)]
            self.last_compact_ms = [0.0] * n
            self.last_records_ms = [float(times.records_ms[i]) for i in range(n)]
            return self.last_times
        return None

    def regen_launch_tables(self):
        """Generate this shard's launch directions and coherent launch order again, ON THE DEVICE
        (hrt_launch_dirs_device, hrt_launch_order_device), and permute the direction table into launch
        order -- what a caller pays per call when the launch set is not kept (bench.py:
        step_incl_launch_ms).  The directions are bit-identical to the host's; results do not depend
        on the order."""
        torch = self.torch
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        if self.order is None:
            raise _lib.HrtError("regen_launch_tables needs a coherent Tracer")
        _lib.check(self.L.hrt_launch_dirs_device(C.byref(self.shard), C.c_void_p(self.dirs.data_ptr()),
                                                 self.device.index, stream, None), "hrt_launch_dirs_device")
        _lib.check(self.L.hrt_launch_order_device(C.byref(self.shard), C.c_void_p(self.order.data_ptr()),
                                                  self.device.index, stream), "hrt_launch_order_device")
        self.dirs_launch = self.dirs[self.order.to(torch.int64) & 0xFFFFFFFF].contiguous()
        self.flags = _lib.DIRS_IN_LAUNCH_ORDER

    # ------------------------------------------------------------------ deferred timing
    def new_timer(self):
        t = C.c_void_p()
        _lib.check(self.L.hrt_timer_create(self.nb, C.byref(t)), "hrt_timer_create")
        return t

    def trace_with_timer(self, timer):
        """Like trace(): asynchronous; HIP events around every kernel go into `timer`."""
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self.L.hrt_trace_flags(
            self.problem, C.byref(self.shard), C.c_void_p(self._dirs_ptr()),
            C.c_void_p(self.order.data_ptr()) if self.order is not None else None,
            C.c_void_p(self.ws.data_ptr()), C.c_uint64(self.ws.numel()), C.c_void_p(stream), timer,
            C.c_uint32(self.flags)), "hrt_trace_flags")
        self._after_trace()

    # ------------------------------------------------------------------ antenna patterns
    def set_patterns(self, rx=None, tx=None, rx_orientation=None, tx_orientation=None):
        """Antenna radiation patterns and orientations of the endpoints (hermespy_rt_amd.patterns; include/hermespy_rt.h
        hrt_pattern): rx / tx a pattern (isotropic(), dipole(), tr38901(), table(values); None: isotropic), one per
        side; rx_orientation / tx_orientation the world -> local rotations, (3, 3) for all endpoints of the side or
        (nrx, 3, 3) / (ntx, 3, 3) (rotation(), look_at(); None: identity).  While patterns are set, trace() and
        trace_with_timer() weight the amplitudes of every unblocked record and every clear LoS entry right after the
        trace, on the same stream (hrt_apply_patterns), so every path-sum member (channel(), taps(), ...) sums the
        weighted paths; paths(), records() and los() show the weighted amplitudes too.  A coincident LoS entry has
        amplitude 1 by definition and is not weighted.  The workspace is not touched here: the patterns hold from the
        next trace() on (or apply_patterns()).  set_patterns() with no arguments removes them.  Invalid arguments
        raise ValueError."""
        from . import patterns as _pt
        if rx is None and tx is None and rx_orientation is None and tx_orientation is None:
            self._patterns = None
            return
        rx, tx = _pt.check(rx), _pt.check(tx)
        rr = _pt.orientations(rx_orientation, self.nrx, "rx_orientation")
        tr = _pt.orientations(tx_orientation, self.ntx, "tx_orientation")
        parts = [a.reshape(-1) for a in (rx["table"], tx["table"], rr, tr) if a is not None]
        torch = self.torch
        with torch.cuda.device(self.device):
            d = torch.from_numpy(np.concatenate(parts + [np.zeros(1, np.float32)])).to(self.device)
        at, ptr = d.data_ptr(), []
        for a in (rx["table"], tx["table"], rr, tr):
            ptr.append(at if a is not None else None)
            at += 0 if a is None else 4 * a.size
        spec = abi.PatternSpec(abi.pattern_struct(rx, ptr[0]), abi.pattern_struct(tx, ptr[1]), ptr[2], ptr[3])
        self._patterns = (spec, d)

    def apply_patterns(self):
        """Weight the current workspace by the stored patterns, on the current stream: for a workspace the caller wrote
        itself after the trace (trace() has applied them already to its own).  RuntimeError if no patterns are set, or
        if the workspace is already weighted since the last trace (applying twice would weight twice)."""
        if self._patterns is None:
            raise RuntimeError("apply_patterns: no patterns are set (set_patterns)")
        if self.patterned:
            raise RuntimeError("apply_patterns: the workspace is already weighted since the last trace")
        self._apply_patterns()

    def _apply_patterns(self):
        spec, d = self._patterns
        stream = self.torch.cuda.current_stream(self.device)
        rc = self.L.hrt_apply_patterns(self.problem, C.byref(self.shard), C.c_void_p(self.ws.data_ptr()),
                                       C.c_uint64(self.ws.numel()), C.byref(spec), C.c_void_p(stream.cuda_stream))
        _lib.check(rc, "hrt_apply_patterns")
        d.record_stream(stream)   # (the kernels read the tables after this call returns)
        self.patterned = True

    def _after_trace(self):
        """what follows every trace on its stream: the patterns, while some are set"""
        self.patterned = False
        if self._patterns is not None:
            self._apply_patterns()

    def debug_last_launch(self):
        """TEST ONLY (hrt_debug_last_launch): run launch nb alone -- the shadow traces and scatter records of bounce
        nb - 1 -- on the live list the caller wrote into hit_block(nb - 1) and counts_tensor()[nb].  Blocks."""
        self.torch.cuda.synchronize(self.device)
        abi.debug_last_launch(self.L, self.problem, self.shard, self.ws.data_ptr(), self.ws.numel())

    def _dirs_ptr(self):
        return (self.dirs_launch if self.flags & _lib.DIRS_IN_LAUNCH_ORDER else self.dirs).data_ptr()

    def read_timer(self, timer, destroy=True):
        """-> dict(los_ms, trace_ms[], shade_ms[], records_ms[], scan_ms[]); waits for the timer's last event."""
        times = _lib.KernelTimes()
        _lib.check(self.L.hrt_timer_read(timer, C.byref(times)), "hrt_timer_read")
        n = int(times.num_bounce_launches)
        out = dict(los_ms=float(times.los_ms), trace_ms=[float(times.trace_ms[i]) for i in range(n)],
                   shade_ms=[float(times.shade_ms[i]) for i in range(n)],
                   records_ms=[float(times.records_ms[i]) for i in range(n)],
                   scan_ms=[0.0] * n)
        if destroy:
            self.L.hrt_timer_destroy(timer)
        return out

    # ------------------------------------------------------------------ views
    def _view(self, off, n, dtype):
        t = self.ws[off:off + n * 4]
        return t.view(dtype)

    def error_word(self):
        """counts[nb + 1] of the last step: 0, or HRT_ERR_* bits (0x100 / 0x200: the step is void, hrt_kparams.h)"""
        return int(self._view(int(self.layout.off_counts), self.nb + 2, self.torch.int32)[self.nb + 1].item()) & 0xFFFFFFFF

    def counts(self, retrace=True):
        """counts[0 .. nb + 1] of the last step (counts[b + 1] = hits of bounce b).  A VOID step -- a fused launch or
        the chain kernel gave up waiting because the GPU is shared (HRT_ERR_FUSE_TIMEOUT / HRT_ERR_CHAIN_TIMEOUT in
        the error word; the library has switched that kernel off for the process by the time this is read) -- is
        traced again here, like the drop-in calls do (retrace=False: raise instead)."""
        torch = self.torch
        for attempt in range(3):
            c = self._view(int(self.layout.off_counts), self.nb + 2, torch.int32).cpu().numpy()
            c = c.astype(np.int64) & 0xFFFFFFFF
            c[0] = self.ntx * self.num_local
            if not (int(c[self.nb + 1]) & 0x300) or not retrace or attempt == 2:   # (hrt_kparams.h: HRT_ERR_VOID)
                break
            self.trace()
        if int(c[self.nb + 1]) & 0x300:
            raise _lib.HrtError("a fused launch timed out waiting for the workgroups in front of it (the GPU is shared "
                                "with other such kernels): this step is void -- trace() again; the library has switched "
                                "to smaller kernels for the rest of the process")
        if c[self.nb + 1] != 0:   # set by the shade kernel if a trace result was out of range
            raise _lib.HrtError("device reported an internal error flag %d" % int(c[self.nb + 1]))
        return c

    def los(self):
        t = self._view(int(self.layout.off_los), self.nrx * self.ntx * _lib.LOS_FLOATS,
                       self.torch.float32)
        return t.cpu().numpy().reshape(self.nrx, self.ntx, _lib.LOS_FLOATS)

    # whole-block views (all `cap` elements), used by sharding.pack_export
    def counts_tensor(self):
        return self._view(int(self.layout.off_counts), self.nb + 2, self.torch.int32)

    def hit_block(self, b):
        base = int(self.layout.off_hits) + b * int(self.layout.hit_block_bytes)
        nf = len(_lib.HIT_FIELDS)
        return self._view(base, nf * self.cap, self.torch.int32).view(nf, self.cap)

    def rec_block(self, b):
        base = int(self.layout.off_recs) + b * int(self.layout.rec_block_bytes)
        nf = len(_lib.REC_FIELDS)
        return self._view(base, self.nrx * nf * self.cap, self.torch.int32).view(self.nrx, nf, self.cap)

    def mask_block(self, b):
        words = self.cap // 64
        moff = int(self.layout.off_masks) + b * self.nrx * words * 8
        return self.ws[moff:moff + self.nrx * words * 8].view(self.torch.int32).view(self.nrx, 2 * words)

    def hits(self, b, n=None):
        """Fields of hit block b (rays that hit at bounce b, state after the bounce)."""
        torch = self.torch
        if n is None:
            n = int(self.counts()[b + 1])
        base = int(self.layout.off_hits) + b * int(self.layout.hit_block_bytes)
        out = {}
        for f, name in enumerate(_lib.HIT_FIELDS):
            dt = torch.int32 if name in ("ray", "tri") else torch.float32
            out[name] = self._view(base + f * self.cap * 4, self.cap, dt)[:n]
        return out

    def records(self, b, n=None):
        """Scatter records of bounce b: dict name -> [nrx, H_b]; 'unblocked' bool [nrx, H_b]."""
        torch = self.torch
        if n is None:
            n = int(self.counts()[b + 1])
        base = int(self.layout.off_recs) + b * int(self.layout.rec_block_bytes)
        nf = len(_lib.REC_FIELDS)
        blk = self._view(base, self.nrx * nf * self.cap, torch.float32).view(self.nrx, nf, self.cap)
        out = {name: blk[:, f, :n] for f, name in enumerate(_lib.REC_FIELDS)}
        words = self.cap // 64
        moff = int(self.layout.off_masks) + b * self.nrx * words * 8
        m = self.ws[moff:moff + self.nrx * words * 8].view(torch.int64).view(self.nrx, words)
        nw = (n + 63) // 64
        bits = (m[:, :nw, None] >> torch.arange(64, device=self.device)) & 1
        out["unblocked"] = bits.reshape(self.nrx, nw * 64)[:, :n].bool()
        return out

    def global_path(self, local_ray):
        """tx, global path index of local ray ids (numpy or torch int tensor)."""
        ch = int(self.shard.chunk) or 4096
        tx = local_ray // self.num_local
        i = local_ray - tx * self.num_local
        p = ((i // ch) * int(self.shard.count) + int(self.shard.rank)) * ch + i % ch
        return tx, p

    def work(self, counts=None):
        """Algorithmic work of the last trace (hrt_stats fields as a dict)."""
        if counts is None:
            counts = self.counts()
        c32 = np.ascontiguousarray(counts, dtype=np.uint32)
        st = _lib.Stats()
        self.L.hrt_work_from_counts(self.problem, C.byref(self.shard),
                                    c32.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(st))
        return dict(live=[int(st.live[i]) for i in range(self.nb + 1)], records=int(st.records),
                    tests=int(st.tests))

    # ------------------------------------------------------------------ path list (COO)
    def paths(self, nonzero_only=True, with_geometry=False):
        """The resolved scatter paths of the last trace as ONE list (device tensors), the form a
        channel model consumes -- instead of the reference's dense [rx][tx][bounce][path] arrays
        of which > 95 % are never written:

            rx, tx, bounce, path   int64 [n]   indices of the dense slot the record belongs to
                                               (path = GLOBAL path index, also on a shard)
            a_te, a_tm             complex64   gains (a blocked record has zeros)
            tau                    float32     delay; direction_rx float32 [n, 3]
            freq_shift             float32     launch Doppler term of the ray minus the record's
                                               (= the dense array's value for one TX; the
                                               reference's dense fill is undefined for more, Q9)
            unblocked              bool        False: blocked record (all-zero gains)
            mesh, face             int64       (with_geometry) triangle the ray left for the RX

        nonzero_only drops the blocked records (the reference writes zeros there)."""
        torch = self.torch
        counts = self.counts()
        cols = {k: [] for k in ("rx", "tx", "bounce", "path", "a_te", "a_tm", "tau", "direction_rx",
                                "freq_shift", "unblocked")}
        if with_geometry:
            cols["mesh"], cols["face"] = [], []
            T = self.num_tri
            mesh_h, face_h = np.empty(T, np.uint32), np.empty(T, np.uint32)
            _lib.check(self.L.hrt_problem_tri_ids(self.problem,
                                                  mesh_h.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                  face_h.ctypes.data_as(C.POINTER(C.c_uint32))),
                       "hrt_problem_tri_ids")
            mesh_d = torch.from_numpy(mesh_h.astype(np.int64)).to(self.device)
            face_d = torch.from_numpy(face_h.astype(np.int64)).to(self.device)
        for b in range(self.nb):
            n = int(counts[b + 1])
            if n == 0:
                continue
            h = self.hits(b, n)
            r = self.records(b, n)
            ray = h["ray"].to(torch.int64) & 0xFFFFFFFF
            tx, p = self.global_path(ray)
            for rx in range(self.nrx):
                ub = r["unblocked"][rx]
                sel = ub if nonzero_only else torch.ones_like(ub)
                k = int(sel.sum().item())
                if k == 0:
                    continue
                cols["rx"].append(torch.full((k,), rx, dtype=torch.int64, device=self.device))
                cols["tx"].append(tx[sel])
                cols["bounce"].append(torch.full((k,), b, dtype=torch.int64, device=self.device))
                cols["path"].append(p[sel])
                cols["a_te"].append(torch.complex(r["a_te_re"][rx][sel], r["a_te_im"][rx][sel]))
                cols["a_tm"].append(torch.complex(r["a_tm_re"][rx][sel], r["a_tm_im"][rx][sel]))
                cols["tau"].append(r["tau"][rx][sel])
                cols["direction_rx"].append(torch.stack([r["dirx"][rx][sel], r["diry"][rx][sel],
                                                         r["dirz"][rx][sel]], dim=1))
                cols["freq_shift"].append(h["fs0"][sel] - r["dfs"][rx][sel])
                cols["unblocked"].append(ub[sel])
                if with_geometry:
                    tri = h["tri"].to(torch.int64)[sel] & 0xFFFFFFFF
                    cols["mesh"].append(mesh_d[tri])
                    cols["face"].append(face_d[tri])
        out = {}
        for k, v in cols.items():
            if v:
                out[k] = torch.cat(v)
            else:
                shape = (0, 3) if k == "direction_rx" else (0,)
                dt = {"a_te": torch.complex64, "a_tm": torch.complex64, "tau": torch.float32,
                      "direction_rx": torch.float32, "freq_shift": torch.float32,
                      "unblocked": torch.bool}.get(k, torch.int64)
                out[k] = torch.empty(shape, dtype=dt, device=self.device)
        return out

    # ------------------------------------------------------------------ channel
    def _pathsum_buffers(self, shape, need, out, accumulate, cache, dtype=None):
        """The output (`out` checked, or a new tensor of `dtype`, default complex64), the scratch cache named `cache`
        grown to `need` bytes and the current stream of one path-sum call (_pathsum)."""
        torch = self.torch
        dtype = torch.complex64 if dtype is None else dtype
        with torch.cuda.device(self.device):
            if out is None:
                if accumulate:
                    raise ValueError("accumulate=True needs `out`")
                out = torch.empty(shape, dtype=dtype, device=self.device)
            elif (tuple(out.shape) != shape or out.dtype != dtype or out.device != self.device
                  or not out.is_contiguous()):
                raise ValueError("out must be a contiguous %s tensor of shape %s on %s"
                                 % (str(dtype).replace("torch.", ""), shape, self.device))
            scratch = getattr(self, cache, None)
            if scratch is None or scratch.numel() < int(need.value):
                scratch = torch.empty(max(int(need.value), 256), dtype=torch.uint8, device=self.device)
                setattr(self, cache, scratch)
        return out, scratch, torch.cuda.current_stream(self.device)

    def _pathsum(self, name, spec, shape, cache, out, accumulate, arrays=None, dtype=None, value_error=True):
        """One call of a path-sum family (`name`: hrt_channel, hrt_array_channel, hrt_taps, hrt_array_taps,
        hrt_power_profiles, hrt_dominant_paths, hrt_beam_channel, hrt_beam_taps or hrt_array_covariance): the scratch
        query, the buffers (scratch cache
        `cache`) and the entry on the current stream.  `arrays`: what _elements prepared for the array families, the
        specs that follow `spec` and last the device tensor they point into.  A spec the library refuses raises
        ValueError, or HrtError where value_error is False."""
        extra = () if arrays is None else tuple(C.byref(a) for a in arrays[:-1])
        need = C.c_uint64(0)
        rc = getattr(self.L, name + "_scratch_bytes")(self.problem, C.byref(self.shard), C.byref(spec), *extra,
                                                      C.byref(need))
        if rc == -1 and value_error:
            raise ValueError(name + ": " + self.L.hrt_last_error().decode())
        _lib.check(rc, name + "_scratch_bytes")
        out, scratch, stream = self._pathsum_buffers(shape, need, out, accumulate, cache, dtype)
        _lib.check(getattr(self.L, name)(self.problem, C.byref(self.shard), C.c_void_p(self.ws.data_ptr()),
                                         C.byref(spec), *extra, C.c_void_p(scratch.data_ptr()),
                                         C.c_uint64(scratch.numel()), C.c_void_p(out.data_ptr()),
                                         1 if accumulate else 0, C.c_void_p(stream.cuda_stream)), name)
        if arrays is not None:
            arrays[-1].record_stream(stream)   # (the kernels read the offsets after this call returns)
        return out

    def _elements(self, rx_elements, tx_elements, array_frequency):
        """The element arguments of an array call, checked -> (Nr, Nt, upload): upload() puts the offsets on the
        device and returns the (ArraySpec, device tensor it points into) that _pathsum takes; with a codebook pair,
        (ArraySpec, BeamSpec, device tensor)."""
        re = abi.elements(rx_elements.cpu().numpy() if hasattr(rx_elements, "cpu") else rx_elements, "rx_elements")
        te = abi.elements(tx_elements.cpu().numpy() if hasattr(tx_elements, "cpu") else tx_elements, "tx_elements")
        if not (np.isfinite(re).all() and np.isfinite(te).all()):
            raise ValueError("element offsets must be finite")
        nr, nt = re.shape[0], te.shape[0]
        fa = self.f_ghz * 1e9 if array_frequency is None else float(array_frequency)

        def upload(weights=None):
            """weights: (W_rx [Br, Nr], W_tx [Bt, Nt]) complex64, uploaded behind the offsets (beam_channel,
            beam_taps)"""
            parts = [re.reshape(-1), te.reshape(-1)]
            if weights is not None:
                parts += [w.view(np.float32).reshape(-1) for w in weights]
            with self.torch.cuda.device(self.device):
                d_el = self.torch.from_numpy(np.concatenate(parts)).to(self.device)
            arrays = abi.ArraySpec(nr, nt, d_el.data_ptr(), d_el.data_ptr() + 12 * nr, fa)
            if weights is None:
                return arrays, d_el
            at = d_el.data_ptr() + 12 * (nr + nt)
            beams = abi.BeamSpec(weights[0].shape[0], weights[1].shape[0], at, at + 8 * weights[0].size)
            return arrays, beams, d_el

        return nr, nt, upload

    def channel(self, f0, df, num_freqs, t0=0.0, dt=0.0, num_times=1, los=True, scatter=True, out=None,
                accumulate=False):
        """Channel frequency response of the last trace, formed on the device (hrt_channel):

            H[rx, tx, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)),  f_k = f0 + k df, t_m = t0 + m dt

        over the LoS entry (los=True; added by shard rank 0 only, so the shards of one launch set sum to the whole
        channel) and every scatter record (scatter=True).  f_k is an absolute frequency (the amplitudes carry no
        carrier phase).  Returns a complex64 tensor [nrx, ntx, 2, num_times, num_freqs] (pol 0 = TE, 1 = TM) on
        the device, enqueued on the current stream; `out` (such a tensor) is written in place, or added to with
        accumulate=True.  The error word is read first (counts()): a void step is traced again."""
        self.counts()
        spec = abi.channel_spec(f0, df, num_freqs, t0, dt, num_times, los, scatter)
        shape = (self.nrx, self.ntx, 2, int(num_times), int(num_freqs))
        return self._pathsum("hrt_channel", spec, shape, "_ch_scratch", out, accumulate, value_error=False)

    def array_channel(self, rx_elements, tx_elements, f0, df, num_freqs, t0=0.0, dt=0.0, num_times=1, los=True,
                      scatter=True, array_frequency=None, out=None, accumulate=False):
        """Antenna-array (MIMO) channel of the last trace, formed on the device (hrt_array_channel):

            H[rx, tx, i, j, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p))
                                               * exp(j 2 pi f_a (r_i . u_p^rx + q_j . u_p^tx) / c)

        rx_elements (Nr, 3) / tx_elements (Nt, 3): element offsets in metres from the traced RX / TX positions (one
        geometry for all RX, one for all TX; numpy or torch), f_a = array_frequency (Hz, default the carrier).  The
        paths and parts are those of channel(); u^rx is the arrival direction (directions_rx), u^tx the departure
        direction (directions_tx for LoS, the launch direction of the ray for a scatter record).  Returns a complex64
        tensor [nrx, ntx, Nr, Nt, 2, num_times, num_freqs] on the device, enqueued on the current stream; `out` is
        written in place, or added to with accumulate=True.  Invalid arguments raise ValueError."""
        nr, nt, upload = self._elements(rx_elements, tx_elements, array_frequency)
        spec = abi.channel_spec(f0, df, num_freqs, t0, dt, num_times, los, scatter)
        self.counts()
        shape = (self.nrx, self.ntx, nr, nt, 2, int(num_times), int(num_freqs))
        return self._pathsum("hrt_array_channel", spec, shape, "_ac_scratch", out, accumulate, upload())

    def beam_channel(self, rx_elements, tx_elements, rx_weights, tx_weights, f0, df, num_freqs, t0=0.0, dt=0.0,
                     num_times=1, los=True, scatter=True, array_frequency=None, out=None, accumulate=False):
        """Beamformed (codebook) channel of the last trace, formed on the device (hrt_beam_channel): the channel after
        the combiner w^H = conj(W_rx[a]) and the precoder f = W_tx[b],

            B[rx, tx, a, b, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)) g_rx[a](u_p^rx) g_tx[b](u_p^tx)
            g_rx[a](u) = sum_i conj(W_rx[a, i]) exp(j 2 pi f_a r_i . u / c)
            g_tx[b](u) = sum_j      W_tx[b, j]  exp(j 2 pi f_a q_j . u / c)

        = sum_ij conj(W_rx[a, i]) H[rx, tx, i, j, pol, m, k] W_tx[b, j] with array_channel()'s H for the same elements,
        without H being formed: the cost follows Br * Bt, not Nr * Nt (hermespy_rt_amd.beams.apply is the host form).
        rx_elements (Nr, 3) / tx_elements (Nt, 3) as in array_channel(); rx_weights (Br, Nr) / tx_weights (Bt, Nt)
        complex (numpy or torch), one codebook for all RX and one for all TX, not normalised.  Returns a complex64
        tensor [nrx, ntx, Br, Bt, 2, num_times, num_freqs] on the device, enqueued on the current stream; `out` is
        written in place, or added to with accumulate=True.  Invalid arguments raise ValueError."""
        nr, nt, upload = self._elements(rx_elements, tx_elements, array_frequency)
        wr = abi.weights(rx_weights.cpu().numpy() if hasattr(rx_weights, "cpu") else rx_weights, nr, "rx_weights")
        wt = abi.weights(tx_weights.cpu().numpy() if hasattr(tx_weights, "cpu") else tx_weights, nt, "tx_weights")
        if not (np.isfinite(wr.view(np.float32)).all() and np.isfinite(wt.view(np.float32)).all()):
            raise ValueError("beam weights must be finite")
        spec = abi.channel_spec(f0, df, num_freqs, t0, dt, num_times, los, scatter)
        self.counts()
        shape = (self.nrx, self.ntx, wr.shape[0], wt.shape[0], 2, int(num_times), int(num_freqs))
        return self._pathsum("hrt_beam_channel", spec, shape, "_bm_scratch", out, accumulate, upload((wr, wt)))

    def taps(self, fs, num_taps, l_min=0, fc=None, t0=0.0, dt=0.0, num_times=1, los=True, scatter=True, out=None,
             accumulate=False):
        """Sampled channel impulse response of the last trace, formed on the device (hrt_taps):

            h[rx, tx, pol, m, i] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) sinc(l_i - f_s tau_p)
            t_m = t0 + m dt,  l_i = l_min + i

        over the paths and parts of channel().  fs is the sampling rate (Hz), fc the frequency the baseband is taken
        around (Hz; None: the carrier, 0 the raw sum).  Its DTFT at |f| < fs / 2 is channel() at fc + f.  Returns a
        complex64 tensor [nrx, ntx, 2, num_times, num_taps] on the device, enqueued on the current stream; `out` is
        written in place, or added to with accumulate=True.  Invalid arguments raise ValueError."""
        fc = self.f_ghz * 1e9 if fc is None else float(fc)
        spec = abi.taps_spec(fs, num_taps, l_min, fc, t0, dt, num_times, los, scatter)
        self.counts()
        shape = (self.nrx, self.ntx, 2, int(num_times), int(num_taps))
        return self._pathsum("hrt_taps", spec, shape, "_tp_scratch", out, accumulate)

    def array_taps(self, rx_elements, tx_elements, fs, num_taps, l_min=0, fc=None, t0=0.0, dt=0.0, num_times=1,
                   los=True, scatter=True, array_frequency=None, out=None, accumulate=False):
        """Antenna-array (MIMO) sampled impulse response of the last trace, formed on the device (hrt_array_taps):

            h[rx, tx, i, j, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p))
                                               * exp(j 2 pi f_a (r_i . u_p^rx + q_j . u_p^tx) / c) sinc(l_k - f_s tau_p)
            t_m = t0 + m dt,  l_k = l_min + k

        the taps of taps() between the elements of array_channel(): rx_elements (Nr, 3) / tx_elements (Nt, 3) element
        offsets in metres (numpy or torch), f_a = array_frequency (Hz), fc the baseband centre (Hz); both default to
        the carrier.  The paths, parts and directions are those of array_channel().  Returns a complex64 tensor
        [nrx, ntx, Nr, Nt, 2, num_times, num_taps] on the device, enqueued on the current stream; `out` is written in
        place, or added to with accumulate=True.  Invalid arguments raise ValueError."""
        nr, nt, upload = self._elements(rx_elements, tx_elements, array_frequency)
        fc = self.f_ghz * 1e9 if fc is None else float(fc)
        spec = abi.taps_spec(fs, num_taps, l_min, fc, t0, dt, num_times, los, scatter)
        self.counts()
        shape = (self.nrx, self.ntx, nr, nt, 2, int(num_times), int(num_taps))
        return self._pathsum("hrt_array_taps", spec, shape, "_at_scratch", out, accumulate, upload())

    def beam_taps(self, rx_elements, tx_elements, rx_weights, tx_weights, fs, num_taps, l_min=0, fc=None, t0=0.0,
                  dt=0.0, num_times=1, los=True, scatter=True, array_frequency=None, out=None, accumulate=False):
        """Beamformed (codebook) sampled impulse response of the last trace, formed on the device (hrt_beam_taps): the
        taps after the combiner w^H = conj(W_rx[a]) and the precoder f = W_tx[b],

            h[rx, tx, a, b, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) g_rx[a](u_p^rx) g_tx[b](u_p^tx)
                                               * sinc(l_k - f_s tau_p),      t_m = t0 + m dt,  l_k = l_min + k

        with beam_channel()'s gains g_rx, g_tx: = sum_ij conj(W_rx[a, i]) h[rx, tx, i, j, pol, m, k] W_tx[b, j] with
        array_taps()'s h for the same elements, without h being formed: the cost follows Br * Bt, not Nr * Nt, and
        Nr * Nt is not limited (hermespy_rt_amd.beams.apply is the host form).  Elements and weights as in
        beam_channel(); fs, num_taps, l_min and fc as in taps().  Returns a complex64 tensor
        [nrx, ntx, Br, Bt, 2, num_times, num_taps] on the device, enqueued on the current stream; `out` is written in
        place, or added to with accumulate=True.  Invalid arguments raise ValueError."""
        nr, nt, upload = self._elements(rx_elements, tx_elements, array_frequency)
        wr = abi.weights(rx_weights.cpu().numpy() if hasattr(rx_weights, "cpu") else rx_weights, nr, "rx_weights")
        wt = abi.weights(tx_weights.cpu().numpy() if hasattr(tx_weights, "cpu") else tx_weights, nt, "tx_weights")
        if not (np.isfinite(wr.view(np.float32)).all() and np.isfinite(wt.view(np.float32)).all()):
            raise ValueError("beam weights must be finite")
        fc = self.f_ghz * 1e9 if fc is None else float(fc)
        spec = abi.taps_spec(fs, num_taps, l_min, fc, t0, dt, num_times, los, scatter)
        self.counts()
        shape = (self.nrx, self.ntx, wr.shape[0], wt.shape[0], 2, int(num_times), int(num_taps))
        return self._pathsum("hrt_beam_taps", spec, shape, "_bt_scratch", out, accumulate, upload((wr, wt)))

    def apply_taps(self, taps, signal, l_min=0, samples_per_block=None, num_out=None, out=None, accumulate=False):
        """Received signals: taps applied to baseband waveforms on the device (hrt_propagate; include/hermespy_rt.h
        hrt_propagate_spec):

            y[rx, i, pol, n] = sum_tx sum_j sum_l taps[rx, tx, i, j, pol, m(n), l] signal[tx, j, n - l_min - l]
            m(n) = min(n // samples_per_block, M - 1),   signal[.., k] = 0 outside 0 <= k < N

        taps: a complex64 device tensor [nrx, ntx, Nr, Nt, 2, M, L] (array_taps(), or beam_taps() with beams for
        elements) or [nrx, ntx, 2, M, L] (taps()); signal: complex64 [ntx, Nt, N] or [ntx, N] on the same device.
        l_min is the l_min the taps were formed with.  samples_per_block=None requires M = 1 (time-invariant);
        num_out defaults to N + L - 1 + max(l_min, 0).  It reads only the two tensors (no trace is needed).  Returns
        a complex64 tensor [nrx, Nr, 2, num_out], enqueued on the current stream; `out` is written in place, or added
        to with accumulate=True.  Invalid arguments raise ValueError."""
        torch = self.torch
        for name, t in (("taps", taps), ("signal", signal)):
            if not (hasattr(t, "is_cuda") and t.is_cuda and t.device == self.device and t.dtype == torch.complex64):
                raise ValueError("%s must be a complex64 tensor on %s" % (name, self.device))
        if taps.dim() == 5:
            taps = taps[:, :, None, None]
        if signal.dim() == 2:
            signal = signal[:, None]
        if taps.dim() != 7 or signal.dim() != 3 or taps.shape[4] != 2:
            raise ValueError("taps [nrx, ntx, Nr, Nt, 2, M, L] (or [nrx, ntx, 2, M, L]) and signal [ntx, Nt, N] (or "
                             "[ntx, N]) expected, got %s and %s" % (tuple(taps.shape), tuple(signal.shape)))
        nrx, ntx, nr, nt, _, m, num_taps = (int(v) for v in taps.shape)
        if (int(signal.shape[0]), int(signal.shape[1])) != (ntx, nt):
            raise ValueError("signal has %d x %d TX ports, the taps %d x %d"
                             % (int(signal.shape[0]), int(signal.shape[1]), ntx, nt))
        n = int(signal.shape[2])
        if samples_per_block is None:
            if m != 1:
                raise ValueError("samples_per_block=None requires taps of one time sample, got %d" % m)
            s = 1
        else:
            s = int(samples_per_block)
        if num_out is None:
            num_out = n + num_taps - 1 + max(int(l_min), 0)
        num_out = int(num_out)
        if not (0 <= s < 1 << 32 and 0 <= num_out < 1 << 62 and -(1 << 31) <= int(l_min) < 1 << 31):
            raise ValueError("samples_per_block, num_out or l_min out of range")
        spec = abi.propagate_spec(nrx, ntx, nr, nt, m, num_taps, l_min, s, n, num_out)
        shape = (nrx, nr, 2, num_out)
        taps, signal = taps.contiguous(), signal.contiguous()
        with torch.cuda.device(self.device):
            if out is None:
                if accumulate:
                    raise ValueError("accumulate=True needs `out`")
                # (an empty output is refused by the library, below: a placeholder it does not write)
                out = torch.empty(shape if nrx * nr * num_out > 0 and num_out <= 1 << 31 else (1,),
                                  dtype=torch.complex64, device=self.device)
            elif (tuple(out.shape) != shape or out.dtype != torch.complex64 or out.device != self.device
                  or not out.is_contiguous()):
                raise ValueError("out must be a contiguous complex64 tensor of shape %s on %s" % (shape, self.device))
            stream = torch.cuda.current_stream(self.device)
        rc = self.L.hrt_propagate(self.device.index, C.byref(spec), C.c_void_p(taps.data_ptr()),
                                  C.c_void_p(signal.data_ptr()), C.c_void_p(out.data_ptr()), 1 if accumulate else 0,
                                  C.c_void_p(stream.cuda_stream))
        if rc == -1:
            raise ValueError("hrt_propagate: " + self.L.hrt_last_error().decode())
        _lib.check(rc, "hrt_propagate")
        taps.record_stream(stream)     # (the kernel reads them after this call returns)
        signal.record_stream(stream)
        return out

    def propagate(self, signal, fs, num_taps, l_min=0, samples_per_block=None, t_start=0.0, rx_elements=None,
                  tx_elements=None, rx_weights=None, tx_weights=None, fc=None, array_frequency=None, num_out=None,
                  los=True, scatter=True, out=None, accumulate=False):
        """The samples the receivers see when the transmitters send `signal` (complex64 [ntx, Nt, N] or [ntx, N] on the
        device, at the rate fs) through the channel of the last trace: what a link-level simulator's
        Channel.propagate(signal) returns, without leaving the device.  It is, bit for bit, apply_taps() of

            beam_taps()   where rx_weights and tx_weights are given (with rx_elements, tx_elements),
            array_taps()  where rx_elements and tx_elements are given,
            taps()        otherwise,

        with num_times = M = ceil(num_out / samples_per_block) blocks formed at their centres, t0 = t_start + (S - 1) /
        (2 fs), dt = S / fs (hermespy_rt_amd.propagate.num_blocks, block_times); samples_per_block=None is the
        time-invariant channel at t_start (M = 1).  num_out defaults to N + num_taps - 1 + max(l_min, 0).  Returns a
        complex64 tensor [nrx, Nr, 2, num_out] (Nr = 1 without elements, Br with weights); `out` is written in place, or
        added to with accumulate=True (the shards of one launch set add up to the whole signal).  Invalid arguments
        raise ValueError."""
        from . import propagate as _pg
        if not hasattr(signal, "dim") or signal.dim() not in (2, 3):
            raise ValueError("signal must be a complex64 tensor [ntx, Nt, N] or [ntx, N] on %s" % (self.device,))
        if num_out is None:
            num_out = _pg.default_num_out(int(signal.shape[-1]), num_taps, l_min)
        m = _pg.num_blocks(num_out, samples_per_block)
        t0, dt = _pg.block_times(fs, samples_per_block, t_start)
        if (rx_weights is None) != (tx_weights is None) or (rx_elements is None) != (tx_elements is None):
            raise ValueError("elements and weights are given for both sides or for neither")
        if rx_weights is not None and rx_elements is None:
            raise ValueError("weights need the elements they apply to")
        kw = dict(l_min=l_min, fc=fc, t0=t0, dt=dt, num_times=m, los=los, scatter=scatter)
        if rx_weights is not None:
            h = self.beam_taps(rx_elements, tx_elements, rx_weights, tx_weights, fs, num_taps,
                               array_frequency=array_frequency, **kw)
        elif rx_elements is not None:
            h = self.array_taps(rx_elements, tx_elements, fs, num_taps, array_frequency=array_frequency, **kw)
        else:
            h = self.taps(fs, num_taps, **kw)
        return self.apply_taps(h, signal, l_min, samples_per_block, num_out, out, accumulate)

    def svd(self, H, vectors=True, out=None):
        """Per-point MIMO SVD of an array channel on the device (hrt_channel_svd; include/hermespy_rt.h
        hrt_compute_channel_svd): for every link, polarisation, time sample and frequency,

            H[rx, tx, :, :, pol, m, k] = u diag(sigma) v^H,   sigma descending, >= 0,   n = min(Nr, Nt)

            sigma   float32   [nrx, ntx, n, 2, T, K]
            u       complex64 [nrx, ntx, Nr, n, 2, T, K]      (None with vectors=False)
            v       complex64 [nrx, ntx, Nt, n, 2, T, K]      (None with vectors=False)
            sweeps  int32     [nrx, ntx, 2, T, K]             Jacobi sweeps that rotated; -1 (abi.SVD_NOT_CONVERGED as a
                                                              signed word) where the cap was reached

        H: a complex64 device tensor [nrx, ntx, Nr, Nt, 2, T, K] (array_channel(), or any tensor of that layout; no
        trace is needed); min(Nr, Nt) <= 16, max(Nr, Nt) <= 64.  One-sided Jacobi in float32: a null column (sigma_i <=
        max(Nr, Nt) 2^-23 sigma_0) has an exactly zero vector on the long side; no gauge beyond sigma >= 0 is fixed.
        The SVD is not additive: the SVD of one shard's partial H is not the channel's, so a sharded caller sums H over
        the shards first and then calls svd().  Returns a dict of views of one flat uint8 device tensor, itself under
        "buffer", enqueued on the current stream; `out` (such a flat tensor) is written in place.
        hermespy_rt_amd.mimo has the host-side reference and what is read from the decomposition.  Invalid arguments
        raise ValueError."""
        torch = self.torch
        if not (hasattr(H, "is_cuda") and H.is_cuda and H.device == self.device and H.dtype == torch.complex64):
            raise ValueError("H must be a complex64 tensor on %s" % (self.device,))
        if H.dim() != 7 or H.shape[4] != 2:
            raise ValueError("H [nrx, ntx, Nr, Nt, 2, T, K] expected, got %s" % (tuple(H.shape),))
        nrx, ntx, nr, nt, _, T, K = (int(v) for v in H.shape)
        spec = abi.svd_spec(nrx, ntx, nr, nt, T, K, vectors)
        H = H.contiguous()
        # (a spec the library refuses may have no sensible size: a placeholder it does not write)
        fits = H.numel() > 0 and 0 < min(nr, nt) <= abi.SVD_MAX_SHORT and max(nr, nt) <= abi.SVD_MAX_LONG
        need = abi.svd_regions(spec)[4] if fits else 1
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty(need, dtype=torch.uint8, device=self.device)
            elif (tuple(out.shape) != (need,) or out.dtype != torch.uint8 or out.device != self.device
                  or not out.is_contiguous()):
                raise ValueError("out must be a contiguous uint8 tensor of shape (%d,) on %s" % (need, self.device))
            stream = torch.cuda.current_stream(self.device)
        rc = self.L.hrt_channel_svd(self.device.index, C.byref(spec), C.c_void_p(H.data_ptr()),
                                    C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream))
        if rc == -1:
            raise ValueError("hrt_channel_svd: " + self.L.hrt_last_error().decode())
        _lib.check(rc, "hrt_channel_svd")
        H.record_stream(stream)     # (the kernel reads it after this call returns)
        return abi.svd_views(out, spec)

    def channel_svd(self, rx_elements, tx_elements, f0, df, num_freqs, t0=0.0, dt=0.0, num_times=1, los=True,
                    scatter=True, array_frequency=None, vectors=True):
        """The per-point MIMO SVD of the last trace's array channel, without leaving the device: bit for bit
        svd(array_channel(...), vectors) with array_channel()'s arguments.  On a sharded trace this is the SVD of the
        shard's partial channel, which is not the channel's: sum array_channel() over the shards and call svd()."""
        H = self.array_channel(rx_elements, tx_elements, f0, df, num_freqs, t0, dt, num_times, los, scatter,
                               array_frequency)
        return self.svd(H, vectors)

    def equalizer(self, H, noise, kind="lmmse", weights=True, out=None):
        """Per-point linear MIMO equalizer of an array channel and its post-equalisation SINR on the device
        (hrt_channel_equalizer; include/hermespy_rt.h hrt_compute_channel_equalizer).  For every link, polarisation,
        time sample and frequency the model is y = H x + n, E[x x^H] = I, E[n n^H] = noise I, H = H[rx, tx, :, :, pol,
        m, k]; with lambda = noise for kind "lmmse", 0 for "zf", and G = (H^H H + lambda I)^-1:

            W       complex64 [nrx, ntx, Nt, Nr, 2, T, K]     G H^H: x_hat = W y           (None with weights=False)
            sinr    float32   [nrx, ntx, Nt, 2, T, K]         1 / (noise G_ii) - [lmmse]   per stream
            status  int32     [nrx, ntx, 2, T, K]             0, abi.EQ_SINGULAR, abi.EQ_NONFINITE

        H: a complex64 device tensor [nrx, ntx, Nr, Nt, 2, T, K] (array_channel(), or any tensor of that layout, such
        as equalize.stack_users() of several links for a multi-user detector; no trace is needed); Nt <= 16, Nr <= 64,
        "zf" needs Nr >= Nt.  `noise`: one finite float > 0.  Modified Gram-Schmidt in float32 on [H; sqrt(lambda) I],
        never through the Gram matrix; a singular or non-finite point writes exact zeros and its status.  The equalizer
        is not additive: the equalizer of one shard's partial H is not the channel's, so a sharded caller sums H over
        the shards first and then calls equalizer().  Returns a dict of views of one flat uint8 device tensor, itself
        under "buffer", enqueued on the current stream; `out` (such a flat tensor) is written in place.
        hermespy_rt_amd.equalize has the host-side reference and what is read from the SINR.  Invalid arguments raise
        ValueError."""
        torch = self.torch
        if not (hasattr(H, "is_cuda") and H.is_cuda and H.device == self.device and H.dtype == torch.complex64):
            raise ValueError("H must be a complex64 tensor on %s" % (self.device,))
        if H.dim() != 7 or H.shape[4] != 2:
            raise ValueError("H [nrx, ntx, Nr, Nt, 2, T, K] expected, got %s" % (tuple(H.shape),))
        nrx, ntx, nr, nt, _, T, K = (int(v) for v in H.shape)
        spec = abi.equalizer_spec(nrx, ntx, nr, nt, T, K, noise, kind, weights)
        H = H.contiguous()
        # (a spec the library refuses may have no sensible size: a placeholder it does not write)
        fits = H.numel() > 0 and 0 < nt <= abi.EQ_MAX_NT and 0 < nr <= abi.EQ_MAX_NR
        need = abi.equalizer_regions(spec)[3] if fits else 1
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty(need, dtype=torch.uint8, device=self.device)
            elif (tuple(out.shape) != (need,) or out.dtype != torch.uint8 or out.device != self.device
                  or not out.is_contiguous()):
                raise ValueError("out must be a contiguous uint8 tensor of shape (%d,) on %s" % (need, self.device))
            stream = torch.cuda.current_stream(self.device)
        rc = self.L.hrt_channel_equalizer(self.device.index, C.byref(spec), C.c_void_p(H.data_ptr()),
                                          C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream))
        if rc == -1:
            raise ValueError("hrt_channel_equalizer: " + self.L.hrt_last_error().decode())
        _lib.check(rc, "hrt_channel_equalizer")
        H.record_stream(stream)     # (the kernel reads it after this call returns)
        return abi.equalizer_views(out, spec)

    def channel_equalizer(self, rx_elements, tx_elements, f0, df, num_freqs, t0=0.0, dt=0.0, num_times=1, los=True,
                          scatter=True, array_frequency=None, noise=1.0, kind="lmmse", weights=True):
        """The per-point equalizer of the last trace's array channel, without leaving the device: bit for bit
        equalizer(array_channel(...), noise, kind, weights) with array_channel()'s arguments.  On a sharded trace this
        is the equalizer of the shard's partial channel, which is not the channel's: sum array_channel() over the
        shards and call equalizer()."""
        H = self.array_channel(rx_elements, tx_elements, f0, df, num_freqs, t0, dt, num_times, los, scatter,
                               array_frequency)
        return self.equalizer(H, noise, kind, weights)

    def precoder(self, H, noise, kind="rzf", power=1.0, regularization=None, normalize="total", weights=True,
                 out=None):
        """Per-point linear MIMO precoder of an array channel and the downlink SINR of every stream behind it, on the
        device (hrt_channel_precoder; include/hermespy_rt.h hrt_compute_channel_precoder).  For every link,
        polarisation, time sample and frequency the model is y = H P s + n, E[s s^H] = I, E[n n^H] = noise I,
        H = H[rx, tx, :, :, pol, m, k]: row i is the channel to stream (user port) i, Nt the transmit elements.
        P0 = H^H for kind "mrt", H^H (H H^H)^-1 for "zf", H^H (H H^H + regularization I)^-1 for "rzf"; normalize "total":
        P = sqrt(power / |P0|_F^2) P0, "stream": column i of P is sqrt(power / Nr) P0[:, i] / |P0[:, i]|:

            P       complex64 [nrx, ntx, Nt, Nr, 2, T, K]     x = P s                         (None with weights=False)
            sinr    float32   [nrx, ntx, Nr, 2, T, K]         |E_ii|^2 / (sum_{j != i} |E_ij|^2 + noise), E = H P
            status  int32     [nrx, ntx, 2, T, K]             0, abi.PC_SINGULAR, abi.PC_NONFINITE

        H: a complex64 device tensor [nrx, ntx, Nr, Nt, 2, T, K] (array_channel(), or any tensor of that layout, such
        as equalize.stack_users(H, "rx") of several users for a multi-user downlink; no trace is needed); Nr <= 16,
        Nt <= 64, "zf" needs Nr <= Nt.  `noise`, `power` and `regularization`: one finite float > 0 each;
        regularization=None under "rzf" is precode.default_regularization(Nr, noise, power) = Nr noise / power.
        Modified Gram-Schmidt in float32 on [H^H; sqrt(regularization) I], never through the Gram matrix; E is formed
        from H and the stored P.  A singular or non-finite point (H = 0 is singular for every kind) writes exact zeros
        and its status.  The precoder is not additive: a sharded caller sums H over the shards first and then calls
        precoder().  Returns a dict of views of one flat uint8 device tensor, itself under "buffer", enqueued on the
        current stream; `out` (such a flat tensor) is written in place.  hermespy_rt_amd.precode has the host-side
        reference and sinr_of() for a P scored through another H.  Invalid arguments raise ValueError."""
        torch = self.torch
        if not (hasattr(H, "is_cuda") and H.is_cuda and H.device == self.device and H.dtype == torch.complex64):
            raise ValueError("H must be a complex64 tensor on %s" % (self.device,))
        if H.dim() != 7 or H.shape[4] != 2:
            raise ValueError("H [nrx, ntx, Nr, Nt, 2, T, K] expected, got %s" % (tuple(H.shape),))
        nrx, ntx, nr, nt, _, T, K = (int(v) for v in H.shape)
        spec = abi.precoder_spec(nrx, ntx, nr, nt, T, K, noise, kind, power, regularization, normalize, weights)
        H = H.contiguous()
        # (a spec the library refuses may have no sensible size: a placeholder it does not write)
        fits = H.numel() > 0 and 0 < nr <= abi.PC_MAX_NR and 0 < nt <= abi.PC_MAX_NT
        need = abi.precoder_regions(spec)[3] if fits else 1
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty(need, dtype=torch.uint8, device=self.device)
            elif (tuple(out.shape) != (need,) or out.dtype != torch.uint8 or out.device != self.device
                  or not out.is_contiguous()):
                raise ValueError("out must be a contiguous uint8 tensor of shape (%d,) on %s" % (need, self.device))
            stream = torch.cuda.current_stream(self.device)
        rc = self.L.hrt_channel_precoder(self.device.index, C.byref(spec), C.c_void_p(H.data_ptr()),
                                         C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream))
        if rc == -1:
            raise ValueError("hrt_channel_precoder: " + self.L.hrt_last_error().decode())
        _lib.check(rc, "hrt_channel_precoder")
        H.record_stream(stream)     # (the kernel reads it after this call returns)
        return abi.precoder_views(out, spec)

    def channel_precoder(self, rx_elements, tx_elements, f0, df, num_freqs, t0=0.0, dt=0.0, num_times=1, los=True,
                         scatter=True, array_frequency=None, noise=1.0, kind="rzf", power=1.0, regularization=None,
                         normalize="total", weights=True):
        """The per-point precoder of the last trace's array channel, without leaving the device: bit for bit
        precoder(array_channel(...), noise, kind, power, regularization, normalize, weights) with array_channel()'s
        arguments.  On a sharded trace this is the precoder of the shard's partial channel, which is not the
        channel's: sum array_channel() over the shards and call precoder()."""
        H = self.array_channel(rx_elements, tx_elements, f0, df, num_freqs, t0, dt, num_times, los, scatter,
                               array_frequency)
        return self.precoder(H, noise, kind, power, regularization, normalize, weights)

    def codebook_select(self, H, codebook, metric="capacity", noise=None, subband=None, table=False, effective=False,
                        out=None):
        """Per-subband precoder codebook selection (the PMI search of limited feedback) on an array channel, on the
        device (hrt_codebook_select; include/hermespy_rt.h hrt_compute_codebook_select).  Every entry W_c of
        `codebook` (complex64 [C, Nt, L], used as given) is scored against the matrices H[rx, tx, :, :, pol, m, k] of a
        subband of `subband` = S consecutive frequencies (None: wideband, S = K; the last subband holds the
        remainder): with E = H_k W_c, metric "power" is the mean of |E|_F^2 over the subband, "capacity" the mean of
        log2 det(I + E^H E / noise).  With B = ceil(K / S):

            index      int32     [nrx, ntx, 2, T, B]          argmax_c, the lowest on a tie (-1: flagged)
            metric     float32   [nrx, ntx, 2, T, B]          its score
            status     int32     [nrx, ntx, 2, T, B]          0, abi.CS_NONFINITE
            table      float32   [nrx, ntx, C, 2, T, B]       every score                      (None without table=True)
            effective  complex64 [nrx, ntx, Nr, L, 2, T, K]   H_k W_c* as it was scored        (None without effective=True)

        `effective` has array_channel()'s layout with Nt = L: equalizer(), svd() and precoder() take it as it is.
        H: a complex64 device tensor [nrx, ntx, Nr, Nt, 2, T, K] (array_channel(), or any tensor of that layout; no
        trace is needed); Nr <= 16, Nt <= 64, L <= min(4, Nt), C <= 4096.  `codebook`: a device tensor or anything
        numpy converts (copied to the device then); hermespy_rt_amd.codebook builds DFT and dual-polarised ones.
        `noise`: one finite float > 0, needed under "capacity".  A subband with a non-finite entry of H or a
        non-finite score writes index -1, metric 0 and zeros.  Selection is not additive: a sharded caller sums H over
        the shards first.  Returns a dict of views of one flat uint8 device tensor, itself under "buffer", enqueued
        on the current stream; `out` (such a flat tensor) is written in place.  Invalid arguments raise ValueError."""
        torch = self.torch
        if not (hasattr(H, "is_cuda") and H.is_cuda and H.device == self.device and H.dtype == torch.complex64):
            raise ValueError("H must be a complex64 tensor on %s" % (self.device,))
        if H.dim() != 7 or H.shape[4] != 2:
            raise ValueError("H [nrx, ntx, Nr, Nt, 2, T, K] expected, got %s" % (tuple(H.shape),))
        nrx, ntx, nr, nt, _, T, K = (int(v) for v in H.shape)
        if hasattr(codebook, "is_cuda"):
            W = codebook
            if W.dim() == 2:
                W = W.unsqueeze(2)
            if not (W.is_cuda and W.device == self.device and W.dtype == torch.complex64 and W.dim() == 3):
                raise ValueError("codebook must be a complex64 tensor [C, Nt, L] on %s" % (self.device,))
        else:
            W = torch.from_numpy(abi.codebook_array(codebook)).to(self.device)
        if int(W.shape[1]) != nt:
            raise ValueError("codebook [C, %d, L] expected, got %s" % (nt, tuple(W.shape)))
        entries, layers = int(W.shape[0]), int(W.shape[2])
        spec = abi.codebook_spec(nrx, ntx, nr, nt, T, K, layers, entries, metric, noise, subband, table, effective)
        H, W = H.contiguous(), W.contiguous()
        # (a spec the library refuses may have no sensible size: a placeholder it does not write)
        fits = H.numel() > 0 and abi.codebook_fits(spec)
        need = abi.codebook_regions(spec)[5] if fits else 1
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty(need, dtype=torch.uint8, device=self.device)
            elif (tuple(out.shape) != (need,) or out.dtype != torch.uint8 or out.device != self.device
                  or not out.is_contiguous()):
                raise ValueError("out must be a contiguous uint8 tensor of shape (%d,) on %s" % (need, self.device))
            stream = torch.cuda.current_stream(self.device)
        rc = self.L.hrt_codebook_select(self.device.index, C.byref(spec), C.c_void_p(H.data_ptr()),
                                        C.c_void_p(W.data_ptr() if W.numel() else None), C.c_void_p(out.data_ptr()),
                                        C.c_void_p(stream.cuda_stream))
        if rc == -1:
            raise ValueError("hrt_codebook_select: " + self.L.hrt_last_error().decode())
        _lib.check(rc, "hrt_codebook_select")
        H.record_stream(stream)     # (the kernel reads them after this call returns)
        W.record_stream(stream)
        return abi.codebook_views(out, spec)

    def channel_codebook_select(self, rx_elements, tx_elements, f0, df, num_freqs, t0=0.0, dt=0.0, num_times=1,
                                los=True, scatter=True, array_frequency=None, codebook=None, metric="capacity",
                                noise=None, subband=None, table=False, effective=False):
        """The codebook selection on the last trace's array channel, without leaving the device: bit for bit
        codebook_select(array_channel(...), codebook, metric, noise, subband, table, effective) with
        array_channel()'s arguments.  On a sharded trace this is the selection on the shard's partial channel, which
        is not the channel's: sum array_channel() over the shards and call codebook_select()."""
        if codebook is None:
            raise ValueError("channel_codebook_select needs a codebook")
        H = self.array_channel(rx_elements, tx_elements, f0, df, num_freqs, t0, dt, num_times, los, scatter,
                               array_frequency)
        return self.codebook_select(H, codebook, metric, noise, subband, table, effective)

    def detect(self, H, Y, constellation, noise, llr=True, out=None):
        """Per-point maximum-likelihood MIMO detection with max-log bit LLRs on an array channel, on the device
        (hrt_channel_detect; include/hermespy_rt.h hrt_compute_channel_detect).  For the point (rx, tx, pol, m, k),
        with H = H[rx, tx, :, :, pol, m, k] (Nr x Nt, Nt streams) and y = Y[rx, tx, :, pol, m, k], every hypothesis
        q < Q = M^Nt -- stream j sends constellation[(q >> (j B)) & (M - 1)], M = 2^B -- is scored by
        d_q = |y - H s(q)|^2:

            index   int32    [nrx, ntx, 2, T, K]          argmin_q d_q, the lowest on a tie (-1: flagged)
            metric  float32  [nrx, ntx, 2, T, K]          its distance
            status  int32    [nrx, ntx, 2, T, K]          0, abi.DT_NONFINITE
            llr     float32  [nrx, ntx, Nt, B, 2, T, K]   (min_{bit 0} d_q - min_{bit 1} d_q) / noise  (None without llr)

        Bit b = 0 of a stream is the most significant bit of its symbol's index; a positive LLR favours bit 1.
        H: a complex64 device tensor [nrx, ntx, Nr, Nt, 2, T, K] (array_channel(), or any tensor of that layout; no
        trace is needed); Y: complex64 [nrx, ntx, Nr, 2, T, K]; Nr <= 64, B <= 8, Nt B <= 12.  `constellation`: a
        device tensor or anything numpy converts (copied to the device then), used as given;
        hermespy_rt_amd.detect builds QAM and PSK ones.  `noise`: one finite float > 0.  A point with a non-finite
        distance or LLR writes index -1, metric 0 and zeros.  Detection is not additive: a sharded caller sums H over
        the shards first.  Returns a dict of views of one flat uint8 device tensor, itself under "buffer", enqueued
        on the current stream; `out` (such a flat tensor) is written in place.  Invalid arguments raise ValueError."""
        torch = self.torch
        if not (hasattr(H, "is_cuda") and H.is_cuda and H.device == self.device and H.dtype == torch.complex64):
            raise ValueError("H must be a complex64 tensor on %s" % (self.device,))
        if H.dim() != 7 or H.shape[4] != 2:
            raise ValueError("H [nrx, ntx, Nr, Nt, 2, T, K] expected, got %s" % (tuple(H.shape),))
        nrx, ntx, nr, nt, _, T, K = (int(v) for v in H.shape)
        if not (hasattr(Y, "is_cuda") and Y.is_cuda and Y.device == self.device and Y.dtype == torch.complex64):
            raise ValueError("Y must be a complex64 tensor on %s" % (self.device,))
        if tuple(Y.shape) != (nrx, ntx, nr, 2, T, K):
            raise ValueError("Y %s expected, got %s" % ((nrx, ntx, nr, 2, T, K), tuple(Y.shape)))
        if hasattr(constellation, "is_cuda"):
            S = constellation
            if not (S.is_cuda and S.device == self.device and S.dtype == torch.complex64 and S.dim() == 1):
                raise ValueError("constellation must be a complex64 tensor [M] on %s" % (self.device,))
        else:
            S = torch.from_numpy(abi.constellation_array(constellation)[0]).to(self.device)
        M = int(S.shape[0])
        if M < 2 or M & (M - 1):
            raise ValueError("constellation must hold 2^B symbols, got %d" % M)
        spec = abi.detect_spec(nrx, ntx, nr, nt, T, K, M.bit_length() - 1, noise, llr)
        H, Y, S = H.contiguous(), Y.contiguous(), S.contiguous()
        # (a spec the library refuses may have no sensible size: a placeholder it does not write)
        fits = H.numel() > 0 and abi.detect_fits(spec)
        need = abi.detect_regions(spec)[4] if fits else 1
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty(need, dtype=torch.uint8, device=self.device)
            elif (tuple(out.shape) != (need,) or out.dtype != torch.uint8 or out.device != self.device
                  or not out.is_contiguous()):
                raise ValueError("out must be a contiguous uint8 tensor of shape (%d,) on %s" % (need, self.device))
            stream = torch.cuda.current_stream(self.device)
        rc = self.L.hrt_channel_detect(self.device.index, C.byref(spec), C.c_void_p(H.data_ptr()),
                                       C.c_void_p(Y.data_ptr() if Y.numel() else None), C.c_void_p(S.data_ptr()),
                                       C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream))
        if rc == -1:
            raise ValueError("hrt_channel_detect: " + self.L.hrt_last_error().decode())
        _lib.check(rc, "hrt_channel_detect")
        H.record_stream(stream)     # (the kernel reads them after this call returns)
        Y.record_stream(stream)
        S.record_stream(stream)
        return abi.detect_views(out, spec)

    def channel_detect(self, rx_elements, tx_elements, f0, df, num_freqs, t0=0.0, dt=0.0, num_times=1, los=True,
                       scatter=True, array_frequency=None, Y=None, constellation=None, noise=None, llr=True):
        """The detection on the last trace's array channel, without leaving the device: bit for bit
        detect(array_channel(...), Y, constellation, noise, llr) with array_channel()'s arguments.  On a sharded
        trace this is the detection on the shard's partial channel, which is not the channel's: sum array_channel()
        over the shards and call detect()."""
        if Y is None or constellation is None or noise is None:
            raise ValueError("channel_detect needs Y, a constellation and the noise power")
        H = self.array_channel(rx_elements, tx_elements, f0, df, num_freqs, t0, dt, num_times, los, scatter,
                               array_frequency)
        return self.detect(H, Y, constellation, noise, llr)

    def kbest(self, H, Y, constellation, noise, k, clip, sorted=True, llr=True, out=None):
        """Per-point K-best tree-search MIMO detection with list max-log bit LLRs on an array channel, on the device
        (hrt_channel_kbest; include/hermespy_rt.h hrt_kbest_spec): near-ML detection at sizes detect() refuses
        (4 x 4 with 16-, 64- or 256-QAM, 8 streams of QPSK or 16-QAM).  H, Y, the constellation, the hypothesis index
        and the bit order are detect()'s.  [H | y] is factored by modified Gram-Schmidt -- sorted QR with
        `sorted` (the weakest residual column first, so the strongest stream is detected first), stream order
        without --, then the tree is walked from the last position, the `k` paths (1, 2, 4, .. 64) of smallest
        partial distance surviving every level, ties to the lower partial hypothesis index:

            index   int32    [nrx, ntx, 2, T, K]          the best leaf of the final list (-1: non-finite; with
                                                          Nt B = 32 a hypothesis reads -1 too: status decides)
            metric  float32  [nrx, ntx, 2, T, K]          its distance |y - H s|^2, comparable with detect()'s
            status  int32    [nrx, ntx, 2, T, K]          0, abi.KB_NONFINITE, abi.KB_DEFICIENT (a null column of
                                                          the QR: rank-deficient H or Nr < Nt; still detected)
            llr     float32  [nrx, ntx, Nt, B, 2, T, K]   (min_{bit 0} - min_{bit 1}) / noise over the final list's
                                                          leaves, clamped to +-clip; a bit whose other value no leaf
                                                          of the list carries gets +-clip  (None without llr)

        Nr <= 64, Nt <= 16, B <= 8, Nt B <= 32.  k = 1 with sorted=True is ordered successive interference
        cancellation; where M^(Nt-1) <= k the decision is the exhaustive one, where M^Nt <= k the LLRs are too.
        Returns a dict of views of one flat uint8 device tensor, itself under "buffer", enqueued on the current
        stream; `out` (such a flat tensor) is written in place.  Invalid arguments raise ValueError."""
        torch = self.torch
        if not (hasattr(H, "is_cuda") and H.is_cuda and H.device == self.device and H.dtype == torch.complex64):
            raise ValueError("H must be a complex64 tensor on %s" % (self.device,))
        if H.dim() != 7 or H.shape[4] != 2:
            raise ValueError("H [nrx, ntx, Nr, Nt, 2, T, K] expected, got %s" % (tuple(H.shape),))
        nrx, ntx, nr, nt, _, T, K = (int(v) for v in H.shape)
        if not (hasattr(Y, "is_cuda") and Y.is_cuda and Y.device == self.device and Y.dtype == torch.complex64):
            raise ValueError("Y must be a complex64 tensor on %s" % (self.device,))
        if tuple(Y.shape) != (nrx, ntx, nr, 2, T, K):
            raise ValueError("Y %s expected, got %s" % ((nrx, ntx, nr, 2, T, K), tuple(Y.shape)))
        if hasattr(constellation, "is_cuda"):
            S = constellation
            if not (S.is_cuda and S.device == self.device and S.dtype == torch.complex64 and S.dim() == 1):
                raise ValueError("constellation must be a complex64 tensor [M] on %s" % (self.device,))
        else:
            S = torch.from_numpy(abi.constellation_array(constellation)[0]).to(self.device)
        M = int(S.shape[0])
        if M < 2 or M & (M - 1):
            raise ValueError("constellation must hold 2^B symbols, got %d" % M)
        if int(k) != k:
            raise ValueError("k must be an integer, got %r" % (k,))
        if not 0 <= int(k) < 1 << 32:
            raise ValueError("k = %r is outside 1 .. 64" % (k,))
        spec = abi.kbest_spec(nrx, ntx, nr, nt, T, K, M.bit_length() - 1, noise, k, clip, sorted, llr)
        H, Y, S = H.contiguous(), Y.contiguous(), S.contiguous()
        # (a spec the library refuses may have no sensible size: a placeholder it does not write)
        fits = H.numel() > 0 and abi.kbest_fits(spec)
        need = abi.kbest_regions(spec)[4] if fits else 1
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.empty(need, dtype=torch.uint8, device=self.device)
            elif (tuple(out.shape) != (need,) or out.dtype != torch.uint8 or out.device != self.device
                  or not out.is_contiguous()):
                raise ValueError("out must be a contiguous uint8 tensor of shape (%d,) on %s" % (need, self.device))
            stream = torch.cuda.current_stream(self.device)
        rc = self.L.hrt_channel_kbest(self.device.index, C.byref(spec), C.c_void_p(H.data_ptr()),
                                      C.c_void_p(Y.data_ptr() if Y.numel() else None), C.c_void_p(S.data_ptr()),
                                      C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream))
        if rc == -1:
            raise ValueError("hrt_channel_kbest: " + self.L.hrt_last_error().decode())
        _lib.check(rc, "hrt_channel_kbest")
        H.record_stream(stream)     # (the kernel reads them after this call returns)
        Y.record_stream(stream)
        S.record_stream(stream)
        return abi.kbest_views(out, spec)

    def channel_kbest(self, rx_elements, tx_elements, f0, df, num_freqs, t0=0.0, dt=0.0, num_times=1, los=True,
                      scatter=True, array_frequency=None, Y=None, constellation=None, noise=None, k=None, clip=None,
                      sorted=True, llr=True):
        """The K-best detection on the last trace's array channel, without leaving the device: bit for bit
        kbest(array_channel(...), Y, constellation, noise, k, clip, sorted, llr) with array_channel()'s arguments.
        On a sharded trace sum array_channel() over the shards and call kbest()."""
        if Y is None or constellation is None or noise is None or k is None or clip is None:
            raise ValueError("channel_kbest needs Y, a constellation, the noise power, k and the clip")
        H = self.array_channel(rx_elements, tx_elements, f0, df, num_freqs, t0, dt, num_times, los, scatter,
                               array_frequency)
        return self.kbest(H, Y, constellation, noise, k, clip, sorted, llr)

    def power_profiles(self, tau0, dtau, num_delay_bins, num_zenith_bins=0, num_azimuth_bins=0, los=True,
                       scatter=True, out=None, accumulate=False):
        """Per-link power statistics of the last trace, formed on the device (hrt_power_profiles): incoherent sums
        of p = |a^pol|^2 over the paths and parts of channel() (include/hermespy_rt.h hrt_compute_power_profiles).

            moments    [nrx, ntx, 2, POWER_FIELDS]  COUNT, P, P_TAU, P_TAU2, P_NU, P_NU2, P_URX_*, P_UTX_*, P_LOS
            pdp        [nrx, ntx, 2, Ld]            p by delay bin floor((tau - tau0) / dtau)
            arrival    [nrx, ntx, 2, Nth, Nph]      p by zenith x azimuth bin of u_rx
            departure  [nrx, ntx, 2, Nth, Nph]      ... of u_tx (the launch direction of a record's ray)

        Returns a dict of float64 views of one flat device tensor, itself under "buffer", enqueued on the current
        stream; `out` (such a flat tensor) is written in place, or added to with accumulate=True.  hermespy_rt_amd.power
        .summarize turns the moments into gains, spreads and K-factors.  Invalid arguments raise ValueError."""
        spec = abi.power_spec(tau0, dtau, num_delay_bins, num_zenith_bins, num_azimuth_bins, los, scatter)
        self.counts()
        shape = (abi.power_out_doubles(self.nrx, self.ntx, spec),)
        out = self._pathsum("hrt_power_profiles", spec, shape, "_pw_scratch", out, accumulate,
                            dtype=self.torch.float64)
        return abi.power_views(out, self.nrx, self.ntx, spec)

    def array_covariance(self, rx_elements=None, tx_elements=None, los=True, scatter=True, array_frequency=None,
                         out=None, accumulate=False):
        """Per-link spatial covariance matrices of an antenna array of the last trace, formed on the device
        (hrt_array_covariance; include/hermespy_rt.h hrt_compute_array_covariance):

            rx  [nrx, ntx, 2, Nr, Nr]   R_rx[i, i'] = sum_p |a_p^pol|^2 s_i(u_p^rx) conj(s_i'(u_p^rx))
            tx  [nrx, ntx, 2, Nt, Nt]   R_tx[j, j'] = sum_p |a_p^pol|^2 t_j(u_p^tx) conj(t_j'(u_p^tx))
            s_i(u) = exp(j 2 pi f_a r_i . u / c),  t_j(u) = exp(j 2 pi f_a q_j . u / c)

        over the terms of power_profiles() with the elements, f_a and steering of array_channel(): with independent
        uniform path phases R_rx = E[H H^H] / Nt and R_tx[j, j'] = E[sum_i H[i, j] conj(H[i, j'])] / Nr.  A side whose
        elements are None is not formed (its view has N = 0).  Exactly Hermitian, with a real diagonal.  Returns a
        dict of complex64 views of one flat device tensor, itself under "buffer", enqueued on the current stream; `out`
        (such a flat tensor) is written in place, or added to with accumulate=True.  hermespy_rt_amd.covariance has the
        host-side reference and what is built on the matrices.  Invalid arguments raise ValueError."""
        none = np.zeros((0, 3), np.float32)
        nr, nt, upload = self._elements(none if rx_elements is None else rx_elements,
                                        none if tx_elements is None else tx_elements, array_frequency)
        spec = abi.covariance_spec(rx_elements is not None, tx_elements is not None, los, scatter)
        self.counts()
        shape = (abi.covariance_out_floats(self.nrx, self.ntx, (nr, nt), spec) // 2,)
        out = self._pathsum("hrt_array_covariance", spec, shape, "_cv_scratch", out, accumulate, upload())
        return abi.covariance_views(out, self.nrx, self.ntx, nr, nt)

    def dominant_paths(self, max_paths, los=True, scatter=True, out=None, accumulate=False):
        """The max_paths strongest paths of every link of the last trace, selected on the device (hrt_dominant_paths;
        include/hermespy_rt.h hrt_dominant_path): the eligible terms are those of channel() (the LoS entry, shard rank
        0 only, and every unblocked scatter record), ranked by the FP64 power |a_te|^2 + |a_tm|^2, ties by bounce
        (LoS: -1) and then by global path, so the list does not depend on shards or on the device's record order.

            kept, eligible                          [nrx, ntx]      records in the list / eligible terms
            power, path, bounce, tri, tau, freq_shift  [nrx, ntx, K]   (tri: row of the device table, tri_order maps it)
            a_te, a_tm                              [nrx, ntx, K]   complex64
            u_rx, u_tx                              [nrx, ntx, K, 3]

        Returns a dict of views of one flat uint8 device tensor (abi.dominant_views), itself under "buffer", enqueued
        on the current stream; the slots past `kept` are zero bytes.  `out` (such a flat tensor) is written in place,
        or, with accumulate=True, MERGED with: the first K of its records and this trace's terms, which is how the
        shards of one launch set combine into the unsharded list.  Invalid arguments raise ValueError."""
        spec = abi.dominant_spec(max_paths, los, scatter)
        self.counts()
        shape = (abi.dominant_out_bytes(self.nrx, self.ntx, spec),)
        out = self._pathsum("hrt_dominant_paths", spec, shape, "_dm_scratch", out, accumulate,
                            dtype=self.torch.uint8)
        return abi.dominant_views(out, self.nrx, self.ntx, spec.max_paths)

    def _path_lists(self, paths):
        """The lists of a sparse call -> (flat uint8 device tensor, nrx, ntx, K): `paths` is a result dict
        (abi.dominant_views: dominant_paths(), dominant.merge, dominant.from_terms), whose "buffer" is read and whose
        views give (nrx, ntx, K), or a flat uint8 buffer of this tracer's (nrx, ntx).  A numpy buffer is uploaded."""
        torch = self.torch
        if isinstance(paths, dict):
            buf = paths["buffer"]
            nrx, ntx, K = (int(v) for v in paths["power"].shape)
        else:
            buf, nrx, ntx = paths, self.nrx, self.ntx
            K = (int(np.prod(buf.shape)) // max(nrx * ntx, 1) - 16) // 72 if hasattr(buf, "shape") else 0
        if isinstance(buf, np.ndarray):
            if buf.dtype != np.uint8:
                raise ValueError("paths: a uint8 buffer expected, got %s" % (buf.dtype,))
        elif not (hasattr(buf, "is_cuda") and buf.dtype == torch.uint8):
            raise ValueError("paths: a uint8 buffer (numpy array or tensor on %s) expected" % (self.device,))
        elif not buf.is_cuda or buf.device != self.device:
            raise ValueError("paths: the buffer must be on %s, got %s" % (self.device, buf.device))
        need = nrx * ntx * (16 + 72 * K)
        if K < 1 or len(buf.shape) != 1 or int(buf.shape[0]) != need:
            raise ValueError("paths: a flat buffer of %d bytes expected for (nrx, ntx, K) = (%d, %d, %d), got %s"
                             % (need, nrx, ntx, K, tuple(buf.shape)))
        if isinstance(buf, np.ndarray):
            with torch.cuda.device(self.device):
                buf = torch.from_numpy(np.ascontiguousarray(buf)).to(self.device)
        elif not buf.is_contiguous():
            raise ValueError("paths: the buffer must be contiguous")
        return buf, nrx, ntx, K

    def sparse_array_channel(self, paths, rx_elements, tx_elements, f0, df, num_freqs, t0=0.0, dt=0.0, num_times=1,
                             array_frequency=None, out=None, accumulate=False):
        """The antenna-array channel of dominant-path lists, formed on the device (hrt_sparse_array_channel;
        include/hermespy_rt.h hrt_compute_sparse_array_channel): with n = min(kept, K) of the link,

            H[rx, tx, i, j, pol, m, k] = sum_{p < n} a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p))
                                                    * exp(j 2 pi f_a (r_i . u_rx_p + q_j . u_tx_p) / c)

        paths: the dict dominant_paths() returns (its "buffer" is read where it is), or a numpy result of
        dominant.merge / dominant.from_terms (uploaded).  The grid, the elements and f_a are array_channel()'s.  No
        trace is needed: only the lists are read, so a traced channel can be evaluated again for another grid, array or
        time axis, and merged or synthetic lists run through the same kernel.  Slots at or beyond n are never read.
        Returns a complex64 tensor [nrx, ntx, Nr, Nt, 2, num_times, num_freqs] on the device, enqueued on the current
        stream; `out` is written in place, or added to with accumulate=True.  Invalid arguments raise ValueError."""
        torch = self.torch
        nr, nt, upload = self._elements(rx_elements, tx_elements, array_frequency)
        buf, nrx, ntx, K = self._path_lists(paths)
        spec = abi.sparse_spec(nrx, ntx, K, f0, df, num_freqs, t0, dt, num_times)
        # (a call the library refuses may have no sensible size: a placeholder it does not write)
        fits = (abi.sparse_out_bytes(spec, nr, nt) > 0 and 0 < nr <= 1024 and 0 < nt <= 1024
                and nr * nt * int(num_times) * int(num_freqs) <= 1 << 24)
        shape = (nrx, ntx, nr, nt, 2, int(num_times), int(num_freqs)) if fits else (1,)
        with torch.cuda.device(self.device):
            if out is None:
                if accumulate:
                    raise ValueError("accumulate=True needs `out`")
                out = torch.empty(shape, dtype=torch.complex64, device=self.device)
            elif (tuple(out.shape) != shape or out.dtype != torch.complex64 or out.device != self.device
                  or not out.is_contiguous()):
                raise ValueError("out must be a contiguous complex64 tensor of shape %s on %s" % (shape, self.device))
            stream = torch.cuda.current_stream(self.device)
        arrays, d_el = upload()
        rc = self.L.hrt_sparse_array_channel(self.device.index, C.byref(spec), C.c_void_p(arrays.rx_elements), nr,
                                             C.c_void_p(arrays.tx_elements), nt, float(arrays.array_frequency_hz),
                                             C.c_void_p(buf.data_ptr()), C.c_void_p(out.data_ptr()),
                                             1 if accumulate else 0, C.c_void_p(stream.cuda_stream))
        if rc == -1:
            raise ValueError("hrt_sparse_array_channel: " + self.L.hrt_last_error().decode())
        _lib.check(rc, "hrt_sparse_array_channel")
        d_el.record_stream(stream)   # (the kernel reads the offsets and the lists after this call returns)
        buf.record_stream(stream)
        return out

    def sparse_channel(self, paths, f0, df, num_freqs, t0=0.0, dt=0.0, num_times=1, out=None, accumulate=False):
        """The SISO channel of dominant-path lists: sparse_array_channel() at one zero-offset element per side, bit for
        bit, as a complex64 tensor [nrx, ntx, 2, num_times, num_freqs] (channel()'s layout)."""
        z = np.zeros((1, 3), np.float32)
        o7 = None
        if out is not None:
            if out.dim() != 5 or not out.is_contiguous():
                raise ValueError("out must be a contiguous complex64 tensor [nrx, ntx, 2, num_times, num_freqs]")
            o7 = out.view(tuple(out.shape[:2]) + (1, 1) + tuple(out.shape[2:]))
        H = self.sparse_array_channel(paths, z, z, f0, df, num_freqs, t0, dt, num_times, 1.0, o7, accumulate)
        return H.view(tuple(H.shape[:2]) + tuple(H.shape[4:])) if out is None else out

    def sparse_beam_channel(self, paths, rx_elements, tx_elements, rx_weights, tx_weights, f0, df, num_freqs, t0=0.0,
                            dt=0.0, num_times=1, array_frequency=None, out=None, accumulate=False):
        """The beamformed (codebook) channel of dominant-path lists, formed on the device (hrt_sparse_beam_channel;
        include/hermespy_rt.h hrt_compute_sparse_beam_channel): with n = min(kept, K) of the link,

            B[rx, tx, a, b, pol, m, k] = sum_{p < n} a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)) g_rx[a](u_rx_p) g_tx[b](u_tx_p)
            g_rx[a](u) = sum_i conj(W_rx[a, i]) exp(j 2 pi f_a r_i . u / c)
            g_tx[b](u) = sum_j      W_tx[b, j]  exp(j 2 pi f_a q_j . u / c)

        = beams.apply(sparse_array_channel(...), W_rx, W_tx) without the element-domain matrix being formed: the cost
        follows Br * Bt, not Nr * Nt, and Nr * Nt is not limited.  paths: what sparse_array_channel() accepts; the
        grid, the elements and f_a are array_channel()'s, the codebooks beam_channel()'s (rx_weights (Br, Nr) applied
        conjugated, tx_weights (Bt, Nt) as they are, not normalised).  No trace is needed: a beam sweep or a codebook
        search over a list costs what the list costs.  Returns a complex64 tensor [nrx, ntx, Br, Bt, 2, num_times,
        num_freqs] on the device, enqueued on the current stream; `out` is written in place, or added to with
        accumulate=True.  Invalid arguments raise ValueError."""
        torch = self.torch
        nr, nt, upload = self._elements(rx_elements, tx_elements, array_frequency)
        wr = abi.weights(rx_weights.cpu().numpy() if hasattr(rx_weights, "cpu") else rx_weights, nr, "rx_weights")
        wt = abi.weights(tx_weights.cpu().numpy() if hasattr(tx_weights, "cpu") else tx_weights, nt, "tx_weights")
        if not (np.isfinite(wr.view(np.float32)).all() and np.isfinite(wt.view(np.float32)).all()):
            raise ValueError("beam weights must be finite")
        br, bt = wr.shape[0], wt.shape[0]
        buf, nrx, ntx, K = self._path_lists(paths)
        spec = abi.sparse_spec(nrx, ntx, K, f0, df, num_freqs, t0, dt, num_times)
        # (a call the library refuses may have no sensible size: a placeholder it does not write)
        fits = (abi.sparse_beam_out_bytes(spec, br, bt) > 0 and 0 < nr <= 256 and 0 < nt <= 256 and 0 < br <= 256
                and 0 < bt <= 256 and br * bt * int(num_times) * int(num_freqs) <= 1 << 24)
        shape = (nrx, ntx, br, bt, 2, int(num_times), int(num_freqs)) if fits else (1,)
        with torch.cuda.device(self.device):
            if out is None:
                if accumulate:
                    raise ValueError("accumulate=True needs `out`")
                out = torch.empty(shape, dtype=torch.complex64, device=self.device)
            elif (tuple(out.shape) != shape or out.dtype != torch.complex64 or out.device != self.device
                  or not out.is_contiguous()):
                raise ValueError("out must be a contiguous complex64 tensor of shape %s on %s" % (shape, self.device))
            stream = torch.cuda.current_stream(self.device)
        arrays, beams_, d_el = upload((wr, wt))
        rc = self.L.hrt_sparse_beam_channel(self.device.index, C.byref(spec), C.c_void_p(arrays.rx_elements), nr,
                                            C.c_void_p(arrays.tx_elements), nt, float(arrays.array_frequency_hz),
                                            C.c_void_p(beams_.rx_weights), br, C.c_void_p(beams_.tx_weights), bt,
                                            C.c_void_p(buf.data_ptr()), C.c_void_p(out.data_ptr()),
                                            1 if accumulate else 0, C.c_void_p(stream.cuda_stream))
        if rc == -1:
            raise ValueError("hrt_sparse_beam_channel: " + self.L.hrt_last_error().decode())
        _lib.check(rc, "hrt_sparse_beam_channel")
        d_el.record_stream(stream)   # (the kernel reads the offsets, the weights and the lists after this call returns)
        buf.record_stream(stream)
        return out

    def sparse_array_taps(self, paths, rx_elements, tx_elements, fs, num_taps, l_min=0, fc=0.0, t0=0.0, dt=0.0,
                          num_times=1, array_frequency=None, out=None, accumulate=False):
        """The antenna-array impulse responses of dominant-path lists, formed on the device (hrt_sparse_array_taps;
        include/hermespy_rt.h hrt_compute_sparse_array_taps): with n = min(kept, K) of the link,

            h[rx, tx, i, j, pol, m, k] = sum_{p < n} a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p))
                                                    * exp(j 2 pi f_a (r_i . u_rx_p + q_j . u_tx_p) / c)
                                                    * sinc(l_min + k - f_s tau_p)

        paths: what sparse_array_channel() accepts (a dominant_paths() result, a merged list, a cluster_list).  fs,
        num_taps, l_min, fc, t0, dt and num_times are array_taps()'s (fc is a number here: no trace, no carrier to
        default to); the elements and f_a are array_channel()'s.  No trace is needed: a traced link can be evaluated
        again for another sampling rate, tap window, array or time axis.  Slots at or beyond n are never read.
        Returns a complex64 tensor [nrx, ntx, Nr, Nt, 2, num_times, num_taps] on the device, enqueued on the current
        stream, which apply_taps() and beams.apply take as it is; `out` is written in place, or added to with
        accumulate=True.  Invalid arguments raise ValueError."""
        torch = self.torch
        nr, nt, upload = self._elements(rx_elements, tx_elements, array_frequency)
        buf, nrx, ntx, K = self._path_lists(paths)
        spec = abi.sparse_taps_spec(nrx, ntx, K, fs, num_taps, l_min, fc, t0, dt, num_times)
        # (a call the library refuses may have no sensible size: a placeholder it does not write)
        fits = (abi.sparse_taps_out_bytes(spec, nr, nt) > 0 and 0 < nr <= 1024 and 0 < nt <= 1024
                and nr * nt * int(num_times) * int(num_taps) <= 1 << 24)
        shape = (nrx, ntx, nr, nt, 2, int(num_times), int(num_taps)) if fits else (1,)
        with torch.cuda.device(self.device):
            if out is None:
                if accumulate:
                    raise ValueError("accumulate=True needs `out`")
                out = torch.empty(shape, dtype=torch.complex64, device=self.device)
            elif (tuple(out.shape) != shape or out.dtype != torch.complex64 or out.device != self.device
                  or not out.is_contiguous()):
                raise ValueError("out must be a contiguous complex64 tensor of shape %s on %s" % (shape, self.device))
            stream = torch.cuda.current_stream(self.device)
        arrays, d_el = upload()
        rc = self.L.hrt_sparse_array_taps(self.device.index, C.byref(spec), C.c_void_p(arrays.rx_elements), nr,
                                          C.c_void_p(arrays.tx_elements), nt, float(arrays.array_frequency_hz),
                                          C.c_void_p(buf.data_ptr()), C.c_void_p(out.data_ptr()),
                                          1 if accumulate else 0, C.c_void_p(stream.cuda_stream))
        if rc == -1:
            raise ValueError("hrt_sparse_array_taps: " + self.L.hrt_last_error().decode())
        _lib.check(rc, "hrt_sparse_array_taps")
        d_el.record_stream(stream)   # (the kernel reads the offsets and the lists after this call returns)
        buf.record_stream(stream)
        return out

    def sparse_beam_taps(self, paths, rx_elements, tx_elements, rx_weights, tx_weights, fs, num_taps, l_min=0, fc=0.0,
                         t0=0.0, dt=0.0, num_times=1, array_frequency=None, out=None, accumulate=False):
        """The beamformed (codebook) impulse responses of dominant-path lists, formed on the device
        (hrt_sparse_beam_taps; include/hermespy_rt.h hrt_compute_sparse_beam_taps): with n = min(kept, K) of the link,

            h[rx, tx, a, b, pol, m, k] = sum_{p < n} a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) g_rx[a](u_rx_p) g_tx[b](u_tx_p)
                                                    * sinc(l_min + k - f_s tau_p)
            g_rx[a](u) = sum_i conj(W_rx[a, i]) exp(j 2 pi f_a r_i . u / c)
            g_tx[b](u) = sum_j      W_tx[b, j]  exp(j 2 pi f_a q_j . u / c)

        = beams.apply(sparse_array_taps(...), W_rx, W_tx) without the element-domain taps being formed: the cost
        follows Br * Bt, not Nr * Nt, and Nr * Nt is not limited.  paths: what sparse_beam_channel() accepts; fs,
        num_taps, l_min, fc, t0, dt and num_times are sparse_array_taps()'s (fc is a number: no trace, no carrier to
        default to); the elements and f_a are array_channel()'s, the codebooks beam_channel()'s (rx_weights (Br, Nr)
        applied conjugated, tx_weights (Bt, Nt) as they are, not normalised).  No trace is needed: a beam sweep in the
        time domain costs what the list costs.  Returns a complex64 tensor [nrx, ntx, Br, Bt, 2, num_times, num_taps]
        on the device, enqueued on the current stream, which apply_taps() takes as it is; `out` is written in place,
        or added to with accumulate=True.  Invalid arguments raise ValueError."""
        torch = self.torch
        nr, nt, upload = self._elements(rx_elements, tx_elements, array_frequency)
        wr = abi.weights(rx_weights.cpu().numpy() if hasattr(rx_weights, "cpu") else rx_weights, nr, "rx_weights")
        wt = abi.weights(tx_weights.cpu().numpy() if hasattr(tx_weights, "cpu") else tx_weights, nt, "tx_weights")
        if not (np.isfinite(wr.view(np.float32)).all() and np.isfinite(wt.view(np.float32)).all()):
            raise ValueError("beam weights must be finite")
        br, bt = wr.shape[0], wt.shape[0]
        buf, nrx, ntx, K = self._path_lists(paths)
        spec = abi.sparse_taps_spec(nrx, ntx, K, fs, num_taps, l_min, fc, t0, dt, num_times)
        # (a call the library refuses may have no sensible size: a placeholder it does not write)
        fits = (abi.sparse_beam_taps_out_bytes(spec, br, bt) > 0 and 0 < nr <= 256 and 0 < nt <= 256 and 0 < br <= 256
                and 0 < bt <= 256 and br * bt * int(num_times) * int(num_taps) <= 1 << 24)
        shape = (nrx, ntx, br, bt, 2, int(num_times), int(num_taps)) if fits else (1,)
        with torch.cuda.device(self.device):
            if out is None:
                if accumulate:
                    raise ValueError("accumulate=True needs `out`")
                out = torch.empty(shape, dtype=torch.complex64, device=self.device)
            elif (tuple(out.shape) != shape or out.dtype != torch.complex64 or out.device != self.device
                  or not out.is_contiguous()):
                raise ValueError("out must be a contiguous complex64 tensor of shape %s on %s" % (shape, self.device))
            stream = torch.cuda.current_stream(self.device)
        arrays, beams_, d_el = upload((wr, wt))
        rc = self.L.hrt_sparse_beam_taps(self.device.index, C.byref(spec), C.c_void_p(arrays.rx_elements), nr,
                                         C.c_void_p(arrays.tx_elements), nt, float(arrays.array_frequency_hz),
                                         C.c_void_p(beams_.rx_weights), br, C.c_void_p(beams_.tx_weights), bt,
                                         C.c_void_p(buf.data_ptr()), C.c_void_p(out.data_ptr()),
                                         1 if accumulate else 0, C.c_void_p(stream.cuda_stream))
        if rc == -1:
            raise ValueError("hrt_sparse_beam_taps: " + self.L.hrt_last_error().decode())
        _lib.check(rc, "hrt_sparse_beam_taps")
        d_el.record_stream(stream)   # (the kernel reads the offsets, the weights and the lists after this call returns)
        buf.record_stream(stream)
        return out

    def sparse_taps(self, paths, fs, num_taps, l_min=0, fc=0.0, t0=0.0, dt=0.0, num_times=1, out=None,
                    accumulate=False):
        """The SISO impulse responses of dominant-path lists: sparse_array_taps() at one zero-offset element per side,
        bit for bit, as a complex64 tensor [nrx, ntx, 2, num_times, num_taps] (taps()'s layout)."""
        z = np.zeros((1, 3), np.float32)
        o7 = None
        if out is not None:
            if out.dim() != 5 or not out.is_contiguous():
                raise ValueError("out must be a contiguous complex64 tensor [nrx, ntx, 2, num_times, num_taps]")
            o7 = out.view(tuple(out.shape[:2]) + (1, 1) + tuple(out.shape[2:]))
        h = self.sparse_array_taps(paths, z, z, fs, num_taps, l_min, fc, t0, dt, num_times, 1.0, o7, accumulate)
        return h.view(tuple(h.shape[:2]) + tuple(h.shape[4:])) if out is None else out

    # ------------------------------------------------------------------ dense (host) view
    def to_dense(self, sentinel_u32=abi.SENTINEL_U32):
        """Assemble the reference's dense [rx][tx][b][p] scatter arrays on the host from the
        compact device result (global path indices; rays of other shards keep the sentinel).
        Slow, for checking only -- the C drop-in compute_paths() has its own dense writer."""
        torch = self.torch
        nrx, ntx, nb, npth = self.nrx, self.ntx, self.nb, self.num_paths
        shp = (nrx, ntx, nb, npth)

        def sent(shape):
            return np.full(shape, sentinel_u32, np.uint32).view(np.float32)

        out = {k: sent(shp) for k in ("a_te_re", "a_te_im", "a_tm_re", "a_tm_im", "tau", "dfs")}
        out["directions_rx"] = sent(shp + (3,))
        hit_tri = np.full((nb, ntx, npth), 0xFFFFFFFF, np.uint32)
        hit_theta = sent((nb, ntx, npth))
        fs0 = sent((nb, ntx, npth))
        state = sent((nb, ntx, npth, 11))
        counts = self.counts()
        for b in range(nb):
            n = int(counts[b + 1])
            if n == 0:
                continue
            h = {k: v.cpu().numpy() for k, v in self.hits(b, n).items()}
            ray = h["ray"].astype(np.int64) & 0xFFFFFFFF
            tx, p = self.global_path(ray)
            hit_tri[b, tx, p] = self.tri_order[h["tri"].view(np.uint32)]   # reference's flat index
            hit_theta[b, tx, p] = h["theta"]
            fs0[b, tx, p] = h["fs0"]
            for k, name in enumerate(("ox", "oy", "oz", "dx", "dy", "dz", "a_te_re", "a_te_im",
                                      "a_tm_re", "a_tm_im", "tau")):
                state[b, tx, p, k] = h[name]
            r = {k: v.cpu().numpy() for k, v in self.records(b, n).items()}
            for rx in range(nrx):
                ub = r["unblocked"][rx]
                for k in ("a_te_re", "a_te_im", "a_tm_re", "a_tm_im", "tau"):
                    out[k][rx, tx, b, p] = r[k][rx]
                out["dfs"][rx, tx[ub], b, p[ub]] = r["dfs"][rx][ub]
                for c, name in enumerate(("dirx", "diry", "dirz")):
                    out["directions_rx"][rx, tx[ub], b, p[ub], c] = r[name][rx][ub]
        out.update(hit_tri=hit_tri, hit_theta=hit_theta, fs0=fs0, state=state, counts=counts)
        return out
