"""Planted workspaces for the path-sum families (Tracer.channel, array_channel, taps, power_profiles).

After a real trace, plant() overwrites every unblocked scatter record (and every clear LoS entry) of the workspace with
values chosen here and returns the planted terms.  The references below then sum values the test wrote itself: every
term counts equally, and one term is far above every tolerance, so a kernel that drops, doubles, misplaces or
mis-polarises a single record fails.  poison() writes values into every slot a kernel must not read.

The planted values make the references exact or FFT-cheap:

    fs = 2^30 Hz, f0 = fc = 3 fs            f tau = 3 n: every carrier phase is a whole number of revolutions
    tau = n / fs, n < 2^16                   exact in float32, fs tau an exact integer (n distinct within a link,
                                             LoS n = 0; keyed=True: n a function of the record's global identity)
    a_te in {1, 2} j^k, a_tm = a_te j / 2    |a|^2 dyadic (TE 1 or 4, TM 1/4 or 1); a swapped polarisation shows
    nu in NUS, FS0 = 0, DFS = -nu            with dt = DT, nu t_m is a whole number of quarter revolutions

Directions stay as traced (tests/power_edges_util.py plants delays and directions on the bin edges of the power
profiles on top of this).  Only plant() and poison() need a device; the rest is plain numpy."""
import numpy as np

FS = 2.0 ** 30                 # sampling rate of the planted delay grid (Hz)
FC = 3.0 * FS                  # carrier: f0 of the channel, fc of the taps
DT = 2.0 ** -12                # time step (s)
NUS = (0.0, 1024.0, -2048.0, 3072.0)   # Doppler shifts (Hz): nu * DT in quarter revolutions
N_MAX = 1 << 16                # delays n < N_MAX
N_KEYED = 1 << 12              # keyed=True: delays n < N_KEYED
C0 = 299792458.0

# workspace field indices (include/hrt_device.h)
HIT_RAY, HIT_FS0 = 0, 3
REC_A_TE_RE, REC_A_TE_IM, REC_A_TM_RE, REC_A_TM_IM, REC_TAU, REC_DIRX, REC_DIRY, REC_DIRZ, REC_DFS = range(9)
LOS_STATUS, LOS_A, LOS_TAU, LOS_DIRX, LOS_DIRY, LOS_DIRZ, LOS_FS = range(7)
LOS_FLOATS = 8

TERM_KEYS = ("rx", "tx", "bounce", "index", "path", "n", "a_te", "a_tm", "tau", "nu", "urx", "utx", "los")


# ------------------------------------------------------------------ the planted values (pure functions)
def mix(*keys):
    """a 64-bit hash of integer arrays (the planted values of a record are functions of it)"""
    h = np.uint64(0x9E3779B97F4A7C15)
    out = np.full(np.broadcast(*keys).shape, h, np.uint64)
    with np.errstate(over="ignore"):
        for k in keys:
            out ^= np.asarray(k).astype(np.uint64) + h + (out << np.uint64(6)) + (out >> np.uint64(2))
            out *= np.uint64(0xBF58476D1CE4E5B9)
            out ^= out >> np.uint64(31)
    return out


def amplitudes(h):
    """a_te in {1, 2} j^k and a_tm = a_te j / 2 from hashes h (complex128)"""
    h = np.asarray(h, np.uint64)
    mag = np.where(h & np.uint64(1), 2.0, 1.0)
    a_te = mag * (1j ** ((h >> np.uint64(1)) & np.uint64(3)).astype(np.int64))
    # (1j ** k is not exact in numpy for k > 1: round the unit to its exact value)
    a_te = np.round(a_te.real) + 1j * np.round(a_te.imag)
    return a_te, a_te * 0.5j


def doppler(h):
    return np.asarray(NUS)[(np.asarray(h, np.uint64) >> np.uint64(3)) & np.uint64(3)]


def delay(n):
    """tau = n / fs as the float32 the workspace holds (exact for n < 2^24)"""
    return (np.asarray(n, np.float64) / FS).astype(np.float32)


def empty_terms():
    t = {k: np.zeros(0, np.int64) for k in ("rx", "tx", "bounce", "index", "path", "n")}
    t.update(a_te=np.zeros(0, np.complex128), a_tm=np.zeros(0, np.complex128), tau=np.zeros(0), nu=np.zeros(0),
             urx=np.zeros((0, 3)), utx=np.zeros((0, 3)), los=np.zeros(0, bool))
    return t


def concat(*ts):
    return {k: np.concatenate([t[k] for t in ts]) for k in TERM_KEYS}


def select(t, sel):
    return {k: t[k][sel] for k in TERM_KEYS}


def synthetic_terms(nrx, ntx, per_link, seed=0, nb=3):
    """a term list as plant() returns it, without a trace: per_link records per link (random bounces, indices and
    directions) plus a LoS term per link (for the CPU tests of the references)"""
    rng = np.random.default_rng(seed)
    parts = []
    for rx in range(nrx):
        for tx in range(ntx):
            m = per_link + 1
            t = empty_terms()
            t["rx"], t["tx"] = np.full(m, rx), np.full(m, tx)
            t["bounce"] = np.concatenate([[-1], np.sort(rng.integers(0, nb, per_link))])
            t["index"] = np.concatenate([[-1], rng.permutation(4 * per_link)[:per_link]])
            t["path"] = np.concatenate([[-1], rng.integers(0, 1 << 20, per_link)])
            t["n"] = np.concatenate([[0], 1 + rng.permutation(per_link)])
            h = mix(rx, tx, t["bounce"], t["path"])
            t["a_te"], t["a_tm"] = amplitudes(h)
            t["a_te"][0] = t["a_tm"][0] = float(1 + (h[0] & np.uint64(1)))
            t["tau"] = delay(t["n"]).astype(np.float64)
            t["nu"] = doppler(h)
            u = rng.normal(size=(m, 3))
            u = (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
            t["urx"], t["utx"] = u, -u[::-1].copy()
            t["los"] = np.arange(m) == 0
            parts.append(t)
    return concat(*parts)


# ------------------------------------------------------------------ planting into a traced workspace
def _mask_bits(tr, b, n):
    """[nrx, n] bool: the unblocked bits of hit block b"""
    m = tr.mask_block(b).cpu().numpy().view(np.uint64)
    bits = (m[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(tr.nrx, -1)[:, :n].astype(bool)


def launch_dirs(tr):
    """departure direction of every global path (hrt_launch_dirs_host of the whole launch set, float64)"""
    import ctypes as C

    from hermespy_rt_amd import lib
    s = lib.Shard(tr.num_paths, 0, 1, 0, tr.nb)
    d = np.empty((tr.num_paths, 3), np.float32)
    lib.check(tr.L.hrt_launch_dirs_host(C.byref(s), d.ctypes.data_as(C.POINTER(C.c_float)), 0))
    return d.astype(np.float64)


def los_view(tr):
    """the LoS entries of the workspace as a [nrx, ntx, LOS_FLOATS] float32 torch view"""
    off = int(tr.layout.off_los)
    return tr.ws[off:off + tr.nrx * tr.ntx * LOS_FLOATS * 4].view(tr.torch.float32).view(tr.nrx, tr.ntx, LOS_FLOATS)


def los_status(tr):
    return los_view(tr)[:, :, LOS_STATUS].cpu().numpy().view(np.uint32).astype(np.int64)


def plant(tr, keyed=False, seed=0):
    """Overwrite the unblocked records and the clear LoS entries of tr's last trace; return the planted terms (a dict
    of numpy arrays, one entry per term, TERM_KEYS; LoS terms have bounce = index = path = -1).  keyed=False: the
    delays n are distinct within a link (a random permutation of 1 .. N_link); keyed=True: every value is a function
    of (rx, tx, global path, bounce) only, so the shards of one launch set plant the same terms as the whole."""
    torch = tr.torch
    torch.cuda.synchronize(tr.device)
    counts = tr.counts()
    rng = np.random.default_rng(seed)
    dirs = launch_dirs(tr)
    blocks = []
    for b in range(tr.nb):
        n = int(counts[b + 1])
        if n == 0:
            continue
        ray = tr.hit_block(b)[HIT_RAY, :n].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        tx, path = tr.global_path(ray)
        ub = _mask_bits(tr, b, n)
        recs = tr.rec_block(b)[:, :, :n].cpu().numpy().view(np.float32).copy()
        blocks.append((b, n, tx, path, ub, recs))
    parts = []
    for b, n, tx, path, ub, recs in blocks:
        for rx in range(tr.nrx):
            i = np.nonzero(ub[rx])[0]
            t = empty_terms()
            t["rx"], t["tx"], t["bounce"] = np.full(i.size, rx), tx[i], np.full(i.size, b)
            t["index"], t["path"] = i, path[i]
            t["urx"] = recs[rx, REC_DIRX:REC_DIRZ + 1, i].reshape(-1, 3).astype(np.float64)
            t["utx"] = dirs[path[i]]
            t["los"] = np.zeros(i.size, bool)
            parts.append(t)
    T = concat(empty_terms(), *parts)
    h = mix(T["rx"], T["tx"], T["path"], T["bounce"])
    T["a_te"], T["a_tm"] = amplitudes(h)
    T["nu"] = doppler(h)
    if keyed:
        T["n"] = 1 + (h >> np.uint64(40)).astype(np.int64) % (N_KEYED - 1)
    else:
        link = T["rx"] * tr.ntx + T["tx"]
        T["n"] = np.zeros(link.size, np.int64)
        for lk in np.unique(link):
            s = np.nonzero(link == lk)[0]
            T["n"][s] = 1 + rng.permutation(s.size)
        assert T["n"].max(initial=0) < N_MAX, "too many records in a link for distinct delays below 2^16"
    T["tau"] = delay(T["n"]).astype(np.float64)

    # write the records back, block by block
    k = 0
    for b, n, tx, path, ub, recs in blocks:
        for rx in range(tr.nrx):
            i = np.nonzero(ub[rx])[0]
            s = slice(k, k + i.size)
            recs[rx, REC_A_TE_RE, i] = T["a_te"][s].real
            recs[rx, REC_A_TE_IM, i] = T["a_te"][s].imag
            recs[rx, REC_A_TM_RE, i] = T["a_tm"][s].real
            recs[rx, REC_A_TM_IM, i] = T["a_tm"][s].imag
            recs[rx, REC_TAU, i] = T["tau"][s]
            recs[rx, REC_DFS, i] = -T["nu"][s]
            k += i.size
        tr.rec_block(b)[:, :, :n] = torch.from_numpy(recs.view(np.int32)).to(tr.device)
        tr.hit_block(b)[HIT_FS0, :n] = 0   # (float 0: the bits 0)
    assert k == T["rx"].size

    # the LoS entries: clear ones planted, coincident ones are a = 1, tau = nu = 0 by definition, blocked ones absent
    L = los_view(tr)
    Lh = L.cpu().numpy().copy()
    status = Lh[:, :, LOS_STATUS].view(np.uint32)
    los = []
    for rx in range(tr.nrx):
        for tx in range(tr.ntx):
            st = int(status[rx, tx])
            if st == 1:
                continue
            t = empty_terms()
            t["rx"], t["tx"] = np.array([rx]), np.array([tx])
            t["bounce"] = t["index"] = t["path"] = np.array([-1])
            t["n"] = np.array([0])
            t["los"] = np.array([True])
            t["tau"] = np.zeros(1)
            if st == 2:
                hl = mix(rx, tx, seed + 7)
                a = 1.0 + float(hl & np.uint64(1))
                nu = float(doppler(hl))
                u = Lh[rx, tx, LOS_DIRX:LOS_DIRZ + 1].astype(np.float64)
                Lh[rx, tx, LOS_A], Lh[rx, tx, LOS_TAU], Lh[rx, tx, LOS_FS] = a, 0.0, nu
            else:
                a, nu, u = 1.0, 0.0, np.array([-1.0, 0.0, 0.0])
            t["a_te"] = t["a_tm"] = np.array([a + 0j])
            t["nu"] = np.array([nu])
            t["utx"], t["urx"] = u[None, :], -u[None, :]
            los.append(t)
    L.copy_(torch.from_numpy(Lh).to(tr.device))
    torch.cuda.synchronize(tr.device)
    return concat(T, *los)


def link_hash(link):
    """the default `where` of plant_single"""
    return mix(link, 0x51C)


def plant_single(tr, tau32_by_link, where=link_hash, nu_by_link=None, only_live_bit=False):
    """One live record per link (tests/test_gpu_sinc_weights.py): after a trace, every link (rx, tx) that has an
    unblocked scatter record gets exactly one with a_te = 1 + 0j, a_tm = 0.5 + 0j, FS0 = 0, DFS = -nu (default 0) and
    tau = tau32_by_link[rx * ntx + tx]: record number where(link) mod N of its N unblocked records, counted block by
    block in index order.  Every other unblocked record keeps its traced tau and has its four amplitude fields zeroed.
    Every LoS entry is forced clear with a = 1, the link's tau and nu; its direction stays as traced (entries that
    were not clear get the coincident convention's).  only_live_bit=True also clears the mask bit of every other
    record, so that the live one is a batch of its own.

    With fc = 0 or t = 0 and nu = 0 the phase of the live record is exactly 0 and its term is a * w: the output tap is
    the kernel's sinc weight bit for bit (TM: half of it; through the LoS route TE = TM = w).

    Returns S: covered [nlinks] bool (links with a live scatter record), block / index [nlinks] (-1: none), ordinal
    (the live record's number among the link's unblocked records) and count (N); retau_single(tr, S, ...) replants
    the delays and Doppler shifts alone."""
    torch = tr.torch
    torch.cuda.synchronize(tr.device)
    counts = tr.counts()
    nl = tr.nrx * tr.ntx
    blocks = []
    per = np.zeros((tr.nrx, tr.ntx), np.int64)
    for b in range(tr.nb):
        n = int(counts[b + 1])
        if n == 0:
            continue
        ray = tr.hit_block(b)[HIT_RAY, :n].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        tx, _ = tr.global_path(ray)
        ub = _mask_bits(tr, b, n)
        blocks.append((b, n, tx, ub, per.copy()))
        for rx in range(tr.nrx):
            per[rx] += np.bincount(tx[ub[rx]], minlength=tr.ntx)
    count = per.reshape(-1)
    links = np.arange(nl)
    pick = np.where(count > 0, np.asarray(where(links), np.uint64) % np.maximum(count, 1).astype(np.uint64), 0)
    pick = pick.astype(np.int64).reshape(tr.nrx, tr.ntx)
    S = dict(covered=count > 0, count=count.copy(), ordinal=np.where(count > 0, pick.reshape(-1), -1),
             block=np.full(nl, -1, np.int64), index=np.full(nl, -1, np.int64))
    for b, n, tx, ub, before in blocks:
        recs = tr.rec_block(b)[:, :, :n].cpu().numpy().view(np.float32).copy()
        keep = np.zeros_like(ub)
        for rx in range(tr.nrx):
            i = np.nonzero(ub[rx])[0]
            recs[rx, REC_A_TE_RE:REC_A_TM_IM + 1, i] = 0.0
            for t in range(tr.ntx):
                it = i[tx[i] == t]
                k = pick[rx, t] - before[rx, t]
                if per[rx, t] and 0 <= k < it.size:
                    lk = rx * tr.ntx + t
                    S["block"][lk], S["index"][lk] = b, it[k]
                    recs[rx, REC_A_TE_RE, it[k]] = 1.0
                    recs[rx, REC_A_TM_RE, it[k]] = 0.5
                    keep[rx, it[k]] = True
        tr.rec_block(b)[:, :, :n] = torch.from_numpy(recs.view(np.int32)).to(tr.device)
        tr.hit_block(b)[HIT_FS0, :n] = 0   # (float 0: the bits 0)
        if only_live_bit:
            _write_mask_bits(tr, b, n, keep)
    assert ((S["block"] >= 0) == S["covered"]).all()

    L = los_view(tr)
    Lh = L.cpu().numpy().copy()
    status = Lh[:, :, LOS_STATUS].view(np.uint32)
    d = Lh[:, :, LOS_DIRX:LOS_DIRZ + 1]
    d[(status != 2) | ~np.isfinite(d).all(axis=-1)] = (-1.0, 0.0, 0.0)
    status[:] = 2
    Lh[:, :, LOS_A] = 1.0
    L.copy_(torch.from_numpy(Lh).to(tr.device))
    retau_single(tr, S, tau32_by_link, nu_by_link)
    return S


def retau_single(tr, S, tau32_by_link, nu_by_link=None):
    """the delays (and Doppler shifts, default 0) of plant_single's live records and LoS entries, replanted"""
    torch = tr.torch
    nl = tr.nrx * tr.ntx
    tau = np.asarray(tau32_by_link, np.float32).reshape(nl)
    nu = np.zeros(nl, np.float32) if nu_by_link is None else np.asarray(nu_by_link, np.float32).reshape(nl)
    bits = lambda a: torch.from_numpy(a.view(np.int32).copy()).to(tr.device)   # noqa: E731
    rx = np.arange(nl) // tr.ntx
    for b in np.unique(S["block"][S["covered"]]):
        s = S["block"] == b
        r, i = torch.from_numpy(rx[s]).to(tr.device), torch.from_numpy(S["index"][s]).to(tr.device)
        blk = tr.rec_block(int(b))
        blk[r, REC_TAU, i] = bits(tau[s])
        blk[r, REC_DFS, i] = bits(-nu[s])
    L = los_view(tr)
    L[:, :, LOS_TAU] = torch.from_numpy(tau.reshape(tr.nrx, tr.ntx)).to(tr.device)
    L[:, :, LOS_FS] = torch.from_numpy(nu.reshape(tr.nrx, tr.ntx)).to(tr.device)
    torch.cuda.synchronize(tr.device)


def _write_mask_bits(tr, b, n, keep):
    """the unblocked bits below n of hit block b := keep [nrx, n]; the bits at and beyond n stay as they are"""
    torch = tr.torch
    pad = (-n) % 64
    bits = np.pad(keep, ((0, 0), (0, pad))).reshape(tr.nrx, -1, 64).astype(np.uint64)
    words = (bits << np.arange(64, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)   # [nrx, ceil(n / 64)]
    m = tr.mask_block(b).view(torch.int64)   # [nrx, cap / 64]
    if n % 64:
        old = m[:, words.shape[1] - 1].cpu().numpy().view(np.uint64)
        words[:, -1] |= old & ~np.uint64((1 << (n % 64)) - 1)
    m[:, :words.shape[1]] = torch.from_numpy(words.view(np.int64)).to(tr.device)


def poison(tr, counts, value):
    """Write `value` (a float) into every slot a path-sum kernel must not read: all record fields where the mask bit
    is 0, every hit and record slot from the block's count up to cap (HRT_HIT_RAY there = 0), every mask bit at and
    beyond the count (= 1), and all fields but the status of blocked and coincident LoS entries.  Returns how many
    slots of each class were written."""
    torch = tr.torch
    torch.cuda.synchronize(tr.device)
    bits = np.array([value], np.float32).view(np.int32)[0]
    hit = dict(blocked_records=0, tail_slots=0, tail_mask_bits=0, los_blocked=0, los_coincident=0)
    for b in range(tr.nb):
        n = int(counts[b + 1])
        cap = tr.cap
        recs = tr.rec_block(b)
        if n:
            ub = torch.from_numpy(_mask_bits(tr, b, n)).to(tr.device)   # [nrx, n]
            r = recs[:, :, :n]
            r.copy_(torch.where(ub[:, None, :], r, torch.full_like(r, int(bits))))
            hit["blocked_records"] += int((~ub).sum().item())
        if n < cap:
            recs[:, :, n:] = int(bits)
            hb = tr.hit_block(b)
            hb[:, n:] = int(bits)
            hb[HIT_RAY, n:] = 0
            hit["tail_slots"] += cap - n
            m = tr.mask_block(b).view(torch.int64)   # [nrx, cap / 64]
            w = n // 64
            if n % 64:
                m[:, w] |= -(1 << (n % 64))    # bits n % 64 .. 63 of the word (two's complement)
                w += 1
            m[:, w:] = -1
            hit["tail_mask_bits"] += tr.nrx * (cap - n)
    L = los_view(tr)
    st = los_status(tr)
    for rx in range(tr.nrx):
        for tx in range(tr.ntx):
            if st[rx, tx] in (0, 1):
                L[rx, tx, 1:] = float(value)
                hit["los_blocked" if st[rx, tx] == 1 else "los_coincident"] += 1
    torch.cuda.synchronize(tr.device)
    return hit


# ------------------------------------------------------------------ the design, checked
def design_errors(T, keyed=False):
    """what is wrong with a planted term list (empty: nothing): integral exact delays, distinct delays per link,
    dyadic powers, the polarisation relation"""
    errs = []
    tau32 = T["tau"].astype(np.float32)
    if not np.array_equal(tau32.astype(np.float64), T["tau"]):
        errs.append("tau not exact in float32")
    x = T["tau"] * FS
    if not np.array_equal(x, np.rint(x)) or not np.array_equal(x.astype(np.int64), T["n"]):
        errs.append("fs tau is not the integer n")
    if T["n"].size and (T["n"].min() < 0 or T["n"].max() >= N_MAX):
        errs.append("n outside [0, 2^16)")
    if not keyed:
        key = (T["rx"] * (int(T["tx"].max(initial=0)) + 1) + T["tx"]) * N_MAX + T["n"]
        if np.unique(key).size != key.size:
            errs.append("n not distinct within a link")
    for pol in ("a_te", "a_tm"):
        p = np.abs(T[pol]) ** 2
        m, e = np.frexp(p)
        if not (np.all(m == 0.5) and np.all(p >= 0.25)):
            errs.append("|%s|^2 not a power of two >= 1/4" % pol)
    s = ~T["los"]
    if not np.array_equal(T["a_tm"][s], T["a_te"][s] * 0.5j):
        errs.append("a_tm != a_te j / 2")
    if not np.all(np.isin(T["nu"], NUS)):
        errs.append("nu outside NUS")
    return errs


# ------------------------------------------------------------------ references (float64 / exact)
def link_of(T, ntx):
    return T["rx"] * ntx + T["tx"]


def cis(ph):
    """exp(j 2 pi ph) in float64, exact where ph is a whole number of quarter revolutions"""
    r = ph - np.rint(ph)
    q = np.rint(4 * r)
    quarter = np.asarray([1, 1j, -1, -1j])[q.astype(np.int64) % 4]
    return np.where(4 * r == q, quarter, np.exp(2j * np.pi * r))


def _phases(T, s, f, t):
    ta, nv = T["tau"][s], T["nu"][s]
    return cis(nv[:, None, None] * t[None, :, None] - f[None, None, :] * ta[:, None, None])


def channel_direct(T, nrx, ntx, f, t, chunk=256):
    """H[rx, tx, pol, m, k] = sum_p a_p exp(j 2 pi (nu_p t_m - f_k tau_p)), float64"""
    f, t = np.asarray(f, np.float64), np.asarray(t, np.float64)
    H = np.zeros((nrx * ntx, 2, t.size, f.size), np.complex128)
    link = link_of(T, ntx)
    for i in range(0, link.size, chunk):
        s = slice(i, i + chunk)
        e = _phases(T, s, f, t).reshape(-1, t.size * f.size)
        for lk in np.unique(link[s]):
            q = link[s] == lk
            for pol, a in enumerate(("a_te", "a_tm")):
                H[lk, pol] += (T[a][s][q] @ e[q]).reshape(t.size, f.size)
    return H.reshape(nrx, ntx, 2, t.size, f.size)


def channel_hist(T, nrx, ntx, K, t):
    """the inverse DFT over k of the planted channel (f0 = FC, df = FS / K): a_p exp(j 2 pi nu_p t_m) at bin n_p"""
    t = np.asarray(t, np.float64)
    H = np.zeros((nrx * ntx, 2, t.size, K), np.complex128)
    link = link_of(T, ntx)
    e = cis(T["nu"][:, None] * t[None, :])   # [p, T]
    for pol, a in enumerate(("a_te", "a_tm")):
        for m in range(t.size):
            np.add.at(H[:, pol, m], (link, T["n"] % K), T[a] * e[:, m])
    return H.reshape(nrx, ntx, 2, t.size, K)


def taps_direct(T, nrx, ntx, fs, fc, L, l_min, t, chunk=256):
    """h[rx, tx, pol, m, i] = sum_p a_p exp(j 2 pi (nu_p t_m - fc tau_p)) sinc(l_min + i - fs tau_p), float64 (the
    sinc exactly 1 / 0 where fs tau is an integer)"""
    t = np.asarray(t, np.float64)
    h = np.zeros((nrx * ntx, 2, t.size, L), np.complex128)
    link = link_of(T, ntx)
    l = l_min + np.arange(L, dtype=np.float64)
    for i in range(0, link.size, chunk):
        s = slice(i, i + chunk)
        e = _phases(T, s, np.array([fc]), t)[:, :, 0]              # [p, T]
        x = fs * T["tau"][s]
        d = l[None, :] - x[:, None]
        w = np.where(d == 0, 1.0, np.where((x == np.rint(x))[:, None], 0.0, np.sinc(d)))   # [p, L]
        for lk in np.unique(link[s]):
            q = link[s] == lk
            for pol, a in enumerate(("a_te", "a_tm")):
                h[lk, pol] += np.einsum("pm,pl->ml", T[a][s][q][:, None] * e[q], w[q])
    return h.reshape(nrx, ntx, 2, t.size, L)


def taps_planted(T, nrx, ntx, L, l_min, t):
    """taps_direct on the planted grid (fs = FS, fc = FC: every fs tau_p = n_p an integer) as a histogram: the term
    a_p exp(j 2 pi nu_p t_m) at tap n_p - l_min where that lies in the window"""
    t = np.asarray(t, np.float64)
    assert np.array_equal(T["tau"] * FS, T["n"].astype(np.float64))
    h = np.zeros((nrx * ntx, 2, t.size, L), np.complex128)
    i = T["n"] - l_min
    ok = (i >= 0) & (i < L)
    link = link_of(T, ntx)[ok]
    e = _phases(select(T, ok), slice(None), np.array([FC]), t)[:, :, 0]   # [p, T]
    for pol, a in enumerate(("a_te", "a_tm")):
        for m in range(t.size):
            np.add.at(h[:, pol, m], (link, i[ok]), T[a][ok] * e[:, m])
    return h.reshape(nrx, ntx, 2, t.size, L)


def array_direct(T, nrx, ntx, rxe, txe, fa, f, t, chunk=256):
    """H[rx, tx, i, j, pol, m, k] = channel_direct's term times exp(j 2 pi fa (r_i . u_rx + q_j . u_tx) / c)"""
    f, t = np.asarray(f, np.float64), np.asarray(t, np.float64)
    rxe, txe = np.asarray(rxe, np.float32).astype(np.float64), np.asarray(txe, np.float32).astype(np.float64)
    nr, nt = rxe.shape[0], txe.shape[0]
    H = np.zeros((nrx * ntx, nr, nt, 2, t.size, f.size), np.complex128)
    link = link_of(T, ntx)
    for i in range(0, link.size, chunk):
        s = slice(i, i + chunk)
        e = _phases(T, s, f, t).reshape(-1, t.size * f.size)
        st = (fa / C0) * ((T["urx"][s] @ rxe.T)[:, :, None] + (T["utx"][s] @ txe.T)[:, None, :])
        g = cis(st).reshape(-1, nr * nt)
        for lk in np.unique(link[s]):
            q = link[s] == lk
            for pol, a in enumerate(("a_te", "a_tm")):
                w = T[a][s][q][:, None] * e[q]
                H[lk, :, :, pol] += (g[q].T @ w).reshape(nr, nt, t.size, f.size)
    return H.reshape(nrx, ntx, nr, nt, 2, t.size, f.size)


def power_exact(T, nrx, ntx, tau0, dtau, Ld):
    """the moments that are exact on planted terms, {field: [nrx, ntx, 2]} (abi.POWER_* indices), and the PDP
    [nrx, ntx, 2, Ld]; float64 sums of dyadic values, exact in any order"""
    from hermespy_rt_amd import abi
    nl = nrx * ntx
    link = link_of(T, ntx)
    p = np.stack([np.abs(T["a_te"]) ** 2, np.abs(T["a_tm"]) ** 2], axis=1)
    tau, nu = T["tau"], T["nu"]
    out = {}
    for f, w in ((abi.POWER_COUNT, np.ones_like(p)), (abi.POWER_P, p), (abi.POWER_P_TAU, p * tau[:, None]),
                 (abi.POWER_P_TAU2, p * (tau * tau)[:, None]), (abi.POWER_P_NU, p * nu[:, None]),
                 (abi.POWER_P_NU2, p * (nu * nu)[:, None]), (abi.POWER_P_LOS, p * T["los"][:, None])):
        out[f] = np.stack([np.bincount(link, weights=w[:, q], minlength=nl) for q in range(2)], axis=1)
        out[f] = out[f].reshape(nrx, ntx, 2)
    x = (tau - tau0) / dtau
    ok = (x >= 0) & (x < Ld)
    pdp = np.zeros((nl, 2, Ld))
    for q in range(2):
        pdp[:, q] = np.bincount(link[ok] * Ld + np.floor(x[ok]).astype(np.int64), weights=p[ok, q],
                                minlength=nl * Ld).reshape(nl, Ld)
    return out, pdp.reshape(nrx, ntx, 2, Ld)


def power_terms(T, nrx, ntx):
    """the term dict of tests/test_gpu_power.py (_reference / _check) from planted terms"""
    return dict(link=link_of(T, ntx), p=np.stack([np.abs(T["a_te"]) ** 2, np.abs(T["a_tm"]) ** 2], axis=1),
                tau=T["tau"], nu=T["nu"], urx=T["urx"], utx=T["utx"], los=T["los"].astype(np.float64),
                nlinks=nrx * ntx)


# ------------------------------------------------------------------ checks (AssertionError naming the terms)
def _who(T, ntx, rx, tx, n=None):
    """the planted terms of link (rx, tx) (at delay n): '(bounce, index)' strings"""
    s = (T["rx"] == rx) & (T["tx"] == tx)
    if n is not None:
        s &= T["n"] == n
    w = ["los" if T["los"][k] else "(b %d, i %d)" % (T["bounce"][k], T["index"][k]) for k in np.nonzero(s)[0][:3]]
    return ", ".join(w) or "empty"


def check_close(got, ref, tol, what, T=None, ntx=None, delay_axis=None):
    """|got - ref| <= tol everywhere; on failure name up to 8 outputs (rx, tx, ..., and the terms at that delay bin
    if delay_axis names the axis of n)"""
    got = np.asarray(got).astype(np.complex128) if np.iscomplexobj(got) else np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    err = np.where(np.isnan(err), np.inf, err)
    bad = np.argwhere(err > tol)
    if bad.size == 0:
        return float(err.max(initial=0.0))
    lines = []
    for ix in bad[np.argsort(-err[tuple(bad.T)])][:8]:
        rx, tx = int(ix[0]), int(ix[1])
        n = int(ix[delay_axis]) if delay_axis is not None else None
        terms = _who(T, ntx, rx, tx, n) if T is not None else ""
        lines.append("  %s: |err| %.3g, got %s want %s  rx %d tx %d terms %s"
                     % (tuple(int(v) for v in ix), err[tuple(ix)], got[tuple(ix)], ref[tuple(ix)], rx, tx, terms))
    raise AssertionError("%s: %d of %d outputs off by more than %g:\n%s"
                         % (what, bad.shape[0], err.size, tol, "\n".join(lines)))


def check_channel_hist(got, T, nrx, ntx, K, t, tol=1e-3):
    """the inverse DFT over k of got [nrx, ntx, 2, T, K] is the planted histogram, within tol per bin"""
    x = np.fft.ifft(np.asarray(got).astype(np.complex128), axis=-1)
    return check_close(x, channel_hist(T, nrx, ntx, K, t), tol, "channel: inverse DFT bins", T, ntx, delay_axis=4)


def check_taps_planted(got, T, nrx, ntx, L, l_min, t, tol=0.0):
    """taps of the planted grid (fs = FS, fc = FC): tap n_p - l_min is that record's term, every other tap 0"""
    ref = taps_planted(T, nrx, ntx, L, l_min, t)
    got = np.asarray(got)
    # name the delay n = l_min + i of a tap: shift the tap axis so that its index is n (window cut at l_min >= 0)
    if l_min >= 0:
        pad = ((0, 0),) * 4 + ((l_min, 0),)
        return check_close(np.pad(got, pad), np.pad(ref, pad), tol, "taps", T, ntx, delay_axis=4)
    return check_close(got, ref, tol, "taps", T, ntx)


def check_power_exact(got, T, nrx, ntx, tau0, dtau, Ld):
    """COUNT, P, P_TAU, P_TAU2, P_NU, P_NU2, P_LOS and every PDP bin equal their float64 references exactly"""
    from hermespy_rt_amd import abi
    names = {abi.POWER_COUNT: "COUNT", abi.POWER_P: "P", abi.POWER_P_TAU: "P_TAU", abi.POWER_P_TAU2: "P_TAU2",
             abi.POWER_P_NU: "P_NU", abi.POWER_P_NU2: "P_NU2", abi.POWER_P_LOS: "P_LOS"}
    M, pdp = power_exact(T, nrx, ntx, tau0, dtau, Ld)
    m = np.asarray(got["moments"], np.float64).reshape(nrx, ntx, 2, -1)
    for f, ref in M.items():
        check_close(m[..., f], ref, 0.0, "power moment " + names[f], T, ntx)
    g = np.asarray(got["pdp"], np.float64).reshape(pdp.shape)
    off = int(round(-tau0 * FS - 0.5)) if dtau == 1.0 / FS else None
    if off is not None and off <= 0:   # bin j holds delay n = j - off: name the terms there
        pad = ((0, 0),) * 3 + ((-off, 0),)
        check_close(np.pad(g, pad), np.pad(pdp, pad), 0.0, "power pdp", T, ntx, delay_axis=3)
    else:
        check_close(g, pdp, 0.0, "power pdp", T, ntx)


# ------------------------------------------------------------------ negative controls
def mutate(T, k, how):
    """T changed in term k: "drop" it, "double" it (counted twice) or "swap" its polarisations"""
    if how == "drop":
        return select(T, np.arange(T["rx"].size) != k)
    if how == "double":
        return concat(T, select(T, np.array([k])))
    if how == "swap":
        U = {key: v.copy() for key, v in T.items()}
        U["a_te"][k], U["a_tm"][k] = T["a_tm"][k], T["a_te"][k]
        return U
    raise ValueError(how)


MUTATIONS = ("drop", "double", "swap")


def control_records(T):
    """indices of two scatter terms to change: the last record of the last non-empty block of the last TX segment,
    and one at a mask-word edge (index 64 k + 63)"""
    s = np.nonzero(~T["los"])[0]
    tx = T["tx"][s].max()
    s = s[T["tx"][s] == tx]
    b = T["bounce"][s].max()
    s = s[T["bounce"][s] == b]
    last = int(s[np.argmax(T["index"][s])])
    edge = np.nonzero(~T["los"] & (T["index"] % 64 == 63))[0]
    assert edge.size, "no planted record at a mask-word edge"
    return [("last", last), ("word_edge", int(edge[0]))]
