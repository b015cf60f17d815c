"""Host side of the K strongest paths per link (Tracer.dominant_paths, hermespy_rt.compute_dominant_paths): the order
of include/hermespy_rt.h (hrt_dominant_path) on term lists and on result dicts, in plain numpy / torch.

    order_key / reference   the order applied to a term list (what the device selection is tested against)
    merge                   the first K of two results of the same shape: what accumulate=True does on the device, for
                            callers that gather the K records of every rank over their own transport
    captured_fraction       how much of a link's power the kept paths carry
"""
import numpy as np

from . import abi

FIELDS = ("power", "path", "bounce", "tri", "a_te", "a_tm", "tau", "freq_shift", "u_rx", "u_tx")
LOS_PATH = np.uint64(0xFFFFFFFFFFFFFFFF)


def term_power(a_te, a_tm):
    """((double)te_re^2 + (double)te_im^2) + ((double)tm_re^2 + (double)tm_im^2) of complex amplitudes"""
    a_te, a_tm = np.asarray(a_te), np.asarray(a_tm)
    f = lambda x: x.astype(np.float64)   # noqa: E731
    return (f(a_te.real) * f(a_te.real) + f(a_te.imag) * f(a_te.imag)) + \
           (f(a_tm.real) * f(a_tm.real) + f(a_tm.imag) * f(a_tm.imag))


def order_key(link, power, bounce, path):
    """the permutation that sorts terms by link, then in the order of the contract: power descending, bounce
    ascending (LoS: -1), path ascending (as unsigned 64-bit: LoS last, though its bounce has decided by then)"""
    path = np.asarray(path).astype(np.int64).view(np.uint64)
    return np.lexsort((path, np.asarray(bounce, np.int64), -np.asarray(power, np.float64), np.asarray(link, np.int64)))


def empty(nrx, ntx, K):
    """an all-zero result (numpy): no eligible term anywhere"""
    return abi.dominant_views(np.zeros(nrx * ntx * (16 + 72 * K), np.uint8), nrx, ntx, K)


def from_terms(link, cols, nrx, ntx, K):
    """the result dict (numpy, abi.dominant_views of a new buffer) of a list of eligible terms: `link` [n] and `cols`
    with every name of FIELDS [n, ...]"""
    out = empty(nrx, ntx, K)
    link = np.asarray(link, np.int64)
    order = order_key(link, cols["power"], cols["bounce"], cols["path"])
    ls = link[order]
    first = np.searchsorted(ls, np.arange(nrx * ntx))
    rank = np.arange(ls.size) - first[ls]
    keep = rank < K
    src, l, r = order[keep], ls[keep], rank[keep]
    for k in FIELDS:
        v = out[k].reshape((nrx * ntx, K) + out[k].shape[3:])
        v[l, r] = np.asarray(cols[k])[src].astype(v.dtype, copy=False)
    n = np.bincount(link, minlength=nrx * ntx)
    out["eligible"][...] = n.reshape(nrx, ntx)
    out["kept"][...] = np.minimum(n, K).reshape(nrx, ntx)
    return out


def reference(terms, nrx, ntx, K):
    """the first K terms of every link of a planted term list (tests/planted.py TERM_KEYS: rx, tx, bounce, path, a_te,
    a_tm, tau, nu, urx, utx, los; LoS terms have bounce = path = -1) as a result dict; `tri` is not part of a term
    list: 0 for a scatter record, UINT32_MAX for a LoS entry"""
    T = terms
    f32 = lambda x: np.asarray(x).astype(np.float32)   # noqa: E731
    a_te, a_tm = np.asarray(T["a_te"]).astype(np.complex64), np.asarray(T["a_tm"]).astype(np.complex64)
    cols = dict(power=term_power(a_te, a_tm), path=np.asarray(T["path"]).astype(np.int64).view(np.uint64),
                bounce=np.asarray(T["bounce"]).astype(np.int32),
                tri=np.where(np.asarray(T["los"], bool), 0xFFFFFFFF, 0).astype(np.uint32), a_te=a_te,
                a_tm=a_tm, tau=f32(T["tau"]), freq_shift=f32(T["nu"]), u_rx=f32(T["urx"]), u_tx=f32(T["utx"]))
    return from_terms(np.asarray(T["rx"]) * ntx + np.asarray(T["tx"]), cols, nrx, ntx, K)


def _numpy(v):
    return v if isinstance(v, np.ndarray) else v.cpu().numpy()


def merge(a, b):
    """the first K of the union of two results (dicts of abi.dominant_views, numpy or torch, same nrx, ntx and K) ->
    a new numpy result; `eligible` adds.  The parts of one launch set merged in any order give the list of the
    whole."""
    A = {k: _numpy(a[k]) for k in FIELDS + ("kept", "eligible")}
    B = {k: _numpy(b[k]) for k in FIELDS + ("kept", "eligible")}
    nrx, ntx, K = A["power"].shape
    assert B["power"].shape == (nrx, ntx, K), "merge: results of different shapes"
    slot = np.arange(K)
    link = np.broadcast_to(np.arange(nrx * ntx).reshape(nrx, ntx, 1), (nrx, ntx, K))
    sel = [slot < np.asarray(X["kept"]).astype(np.int64)[..., None] for X in (A, B)]
    cols = {}
    for k in FIELDS:
        parts = [X[k].view(np.uint64) if k == "path" else (X[k].view(np.uint32) if k == "tri" else X[k])
                 for X in (A, B)]
        cols[k] = np.concatenate([p[s] for p, s in zip(parts, sel)])
    out = from_terms(np.concatenate([link[s] for s in sel]), cols, nrx, ntx, K)
    out["eligible"][...] = A["eligible"].astype(np.int64).view(np.uint64) + B["eligible"].astype(np.int64).view(np.uint64)
    return out


def captured_fraction(views, moments):
    """kept power over the link's whole power, [nrx, ntx] (nan where the link has none): `views` a result of
    dominant_paths, `moments` the moments of power_profiles for the same parts (POWER_P of both polarisations)"""
    power, kept = _numpy(views["power"]), _numpy(views["kept"]).astype(np.int64)
    m = _numpy(moments)
    total = m[..., 0, abi.POWER_P] + m[..., 1, abi.POWER_P]
    got = np.where(np.arange(power.shape[-1]) < kept[..., None], power, 0.0).sum(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(total > 0, got / total, np.nan)
