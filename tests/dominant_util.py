"""What the tests of the dominant paths (Tracer.dominant_paths, hrt_compute_dominant_paths) share: the expected buffer
built in numpy from Tracer.paths(), Tracer.los() and the hit blocks, and the byte comparison that names the field."""
import numpy as np

from hermespy_rt_amd import dominant

from . import planted as PL
from .pathsum_util import _los_status


def trace_terms(tr, los=True, scatter=True):
    """link [n] and the columns of dominant.FIELDS [n, ...] of every eligible term of tr's last trace: the scatter
    records from Tracer.paths(nonzero_only=True), u_tx from the host's launch directions, tri (rows of the device
    table) from the hit blocks; the LoS entries (rank 0) from Tracer.los()"""
    links, cols = [], {k: [] for k in dominant.FIELDS}
    if scatter:
        P = {k: v.cpu().numpy() for k, v in tr.paths(nonzero_only=True, with_geometry=False).items()}
        dirs = PL.launch_dirs(tr).astype(np.float32)
        counts = tr.counts()
        tri = []
        for b in range(tr.nb):   # (the order of Tracer.paths: bounce, rx, hit)
            n = int(counts[b + 1])
            if n == 0:
                continue
            t = tr.hits(b, n)["tri"].cpu().numpy().view(np.uint32)
            ub = tr.records(b, n)["unblocked"].cpu().numpy()
            tri += [t[ub[rx]] for rx in range(tr.nrx)]
        tri = np.concatenate(tri) if tri else np.zeros(0, np.uint32)
        assert tri.size == P["rx"].size and P["unblocked"].all()
        links.append(P["rx"] * tr.ntx + P["tx"])
        cols["power"].append(dominant.term_power(P["a_te"], P["a_tm"]))
        cols["path"].append(P["path"].astype(np.uint64))
        cols["bounce"].append(P["bounce"].astype(np.int32))
        cols["tri"].append(tri)
        cols["a_te"].append(P["a_te"])
        cols["a_tm"].append(P["a_tm"])
        cols["tau"].append(P["tau"])
        cols["freq_shift"].append(P["freq_shift"])
        cols["u_rx"].append(P["direction_rx"])
        cols["u_tx"].append(dirs[P["path"]])
    if los and tr.shard.rank == 0:
        L = tr.los()
        for rx in range(tr.nrx):
            for tx in range(tr.ntx):
                q = L[rx, tx]
                status = _los_status(q)
                if status == 1:
                    continue
                a, tau, nu, u = np.float32(1), np.float32(0), np.float32(0), np.array([-1, 0, 0], np.float32)
                if status == 2:
                    a, tau, nu, u = q[1], q[2], q[6], q[3:6].copy()
                amp = np.array([complex(a, 0)], np.complex64)
                links.append(np.array([rx * tr.ntx + tx]))
                cols["power"].append(dominant.term_power(amp, amp))
                cols["path"].append(np.array([dominant.LOS_PATH]))
                cols["bounce"].append(np.array([-1], np.int32))
                cols["tri"].append(np.array([0xFFFFFFFF], np.uint32))
                cols["a_te"].append(amp)
                cols["a_tm"].append(amp)
                cols["tau"].append(np.array([tau], np.float32))
                cols["freq_shift"].append(np.array([nu], np.float32))
                cols["u_rx"].append(-u[None, :])
                cols["u_tx"].append(u[None, :])
    if not links:
        return np.zeros(0, np.int64), None
    return np.concatenate(links).astype(np.int64), {k: np.concatenate(v) for k, v in cols.items()}


def expected(tr, K, los=True, scatter=True, terms=None):
    link, cols = trace_terms(tr, los, scatter) if terms is None else terms
    if cols is None:
        return dominant.empty(tr.nrx, tr.ntx, K)
    return dominant.from_terms(link, cols, tr.nrx, tr.ntx, K)


def to_numpy(d):
    """a result dict of torch views as numpy views of ONE host copy of the buffer"""
    from hermespy_rt_amd import abi
    buf = d["buffer"]
    buf = buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()
    nrx, ntx, K = d["power"].shape
    return abi.dominant_views(buf, nrx, ntx, K)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape + (-1,)) if a.dtype.itemsize > 1 else a


def check_bytes(got, want, what=""):
    """got == want, byte for byte: the header, every field of every slot (the zero tail included), the whole buffer.
    On a difference the AssertionError names the first field and slot."""
    got, want = to_numpy(got), to_numpy(want)
    assert got["buffer"].size == want["buffer"].size, (what, got["buffer"].size, want["buffer"].size)
    for k in ("kept", "eligible") + dominant.FIELDS:
        g, w = _bits(got[k]), _bits(want[k])
        if not np.array_equal(g, w):
            bad = np.argwhere((g != w).reshape(got[k].shape + (-1,)).any(axis=-1) if g.ndim > got[k].ndim else g != w)
            ix = tuple(int(v) for v in bad[0])
            raise AssertionError("%s: %s differs in %d places, first at %s: got %r want %r (kept %s / %s)"
                                 % (what, k, bad.shape[0], ix, got[k][ix], want[k][ix],
                                    got["kept"][ix[:2]], want["kept"][ix[:2]]))
    assert np.array_equal(got["buffer"], want["buffer"]), (what, "bytes outside the fields differ")
