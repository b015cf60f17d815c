"""What tests/test_dominant_order_design.py (CPU) and tests/test_gpu_dominant_order.py share: workspaces planted with
exact, distinct powers in a chosen ORDER of the selection's walk, and a model of the slot mechanics of the three
kernels of csrc/hrt_dominant.hip that says which of their edges a case reaches.

    describe / synthetic   what the selection sees of a workspace (W): the TX segments, paths, triangles and arrival
                           directions of the hit blocks and the LoS entries, from a traced Tracer or made up (CPU)
    values / live_bits     the planted value v (power v^2, v an integer < 2^24) and the unblocked bit of every record
    terms / plant_order    the term list (planted.TERM_KEYS) of a planted W, and the planting itself (device)
    plan_of / plan         dm_plan of csrc/host/channel.c: nchunks, nmid and the scratch bytes
    chunk_terms / model    the terms as the workgroups walk them, and the walk: dm_room, the push rule, dm_flush,
                           dm_stream, the final kernel's order; `wrong=` makes one of WRONG's misreadings
    SURVIVORS              the (case, order, live, K) the GPU file runs (the design test derives and checks it)

The model works on a step's candidates at once (numpy), never per record.  What it cannot know is the order the LDS
counter hands the pending slots out in; with a correct dm_room that order decides nothing."""
import numpy as np

from hermespy_rt_amd import dominant

from . import planted as PL
from . import scenes_gen as G

U64 = np.uint64
N = 2048                     # HRT_DM_SLOTS
FANIN = 16                   # HRT_DM_FANIN
MAX_CHUNKS = FANIN * FANIN   # HRT_DM_MAX_CHUNKS
MIN_CHUNK = 512              # HRT_CH_MIN_CHUNK
TARGET_GROUPS = 2048         # HRT_DM_TARGET_GROUPS
PARTIAL_MAX = 512 << 20      # HRT_DM_PARTIAL_MAX
PARTIAL_STEP = 512           # records a step of the partial kernel offers (2 per thread)
MERGE_STEP = 256             # candidates a step of the merge kernel offers
FINAL_STEP = 1024            # ... of the final kernel
PATH_BITS = 48
HIT_TRI = 1

ORDERS = ("asc", "desc", "chunk_asc_record_desc", "middle_chunk", "shuffled")
LIVES = ("all", "odd", "runs")
RUN_ON, RUN_PERIOD = 70, 128   # `runs`: 70 on, 58 off (the period divides neither 64 nor 512 into whole runs)
KS_ALL = (1, 2, 3, 511, 512, 513, 1023, 1024)
KS_BIG = (512, 1023, 1024)
WRONG = ("room_ge", "room_late", "thr_ge", "thr_gt_hi", "hi_only_sort", "merge_unclamped", "merge_skips_last",
         "final_reads_la", "count_not_summed", "old_in_place", "kept_unclamped")

RX2 = [[3.0, 2.0, 1.5], [-5.0, 4.0, 2.0]]
TX2 = [[-10.0, -6.0, 3.0], [12.0, 5.0, 4.0]]
# name: rays per TX, receivers, transmitters, K values, nchunks and nmid the case is named for
CASES = {
    "one_chunk": dict(rays=600, nrx=1, ntx=1, ks=KS_ALL, nchunks=1, nmid=0),
    "fanin_full": dict(rays=8200, nrx=1, ntx=1, ks=KS_ALL, nchunks=16, nmid=0),
    "merge_tail_one": dict(rays=8750, nrx=1, ntx=1, ks=KS_ALL, nchunks=17, nmid=2),
    "merge_two_full": dict(rays=16400, nrx=1, ntx=1, ks=KS_ALL, nchunks=32, nmid=2),
    "cap_1024": dict(rays=262144, nrx=1, ntx=1, ks=KS_BIG, nchunks=256, nmid=16),
    "cap_1536": dict(rays=393216, nrx=1, ntx=1, ks=KS_BIG, nchunks=256, nmid=16),
    "two_by_two": dict(rays=8750, nrx=2, ntx=2, ks=KS_ALL, nchunks=17, nmid=2),
}
BIG = ("cap_1024", "cap_1536")
NB = 2


def combos(case):
    """every (order, live) a case is modelled with: every order with all records live, `asc` and `shuffled` also with
    `odd` and `runs`.  The two 256-chunk cases are there for their chunk size: they leave out `middle_chunk`, `odd`
    and `shuffled` with `runs`, which the 17- and 32-chunk cases reach with the same merge tree."""
    if case in BIG:
        return [("asc", "all"), ("desc", "all"), ("chunk_asc_record_desc", "all"), ("shuffled", "all"), ("asc", "runs")]
    return [(o, "all") for o in ORDERS] + [(o, l) for o in ("asc", "shuffled") for l in ("odd", "runs")]


def config(case, tmp_path_factory):
    """the empty closed room (12 triangles), the endpoints inside, two bounces"""
    c = CASES[case]
    p = str(tmp_path_factory.mktemp("dominant_order") / "room.hrt")
    assert G.room_with_clutter(p, 0) == 12
    return G.cfg(p, RX2[:c["nrx"]], TX2[:c["ntx"]], c["rays"], NB)


# ------------------------------------------------------------------ the plan (dm_plan of csrc/host/channel.c)
def _align256(x):
    return (x + 255) // 256 * 256


def plan_of(num_local, nb, nrx, ntx, K):
    links = nrx * ntx
    per_chunk = links * (K * 24 + 8)
    nch = 0
    if nb > 0:
        nch = max(1, min(-(-TARGET_GROUPS // links), num_local // MIN_CHUNK, PARTIAL_MAX // per_chunk, MAX_CHUNKS))
    nmid = -(-nch // FANIN) if nch > FANIN else 0
    seg = _align256(nb * (ntx + 1) * 4)
    nbytes = (seg + _align256(links * nch * K * 24) + _align256(links * nch * 8) + _align256(links * nmid * K * 24)
              + _align256(links * nmid * 8))
    return dict(nchunks=nch, nmid=nmid, bytes=nbytes)


def plan(tr, K):
    return plan_of(tr.num_local, tr.nb, tr.nrx, tr.ntx, K)


def chunk_starts(n, nchunks):
    """the offsets within a TX segment of n records where the chunks start (chunk_range of csrc/hrt_pathsum.h)"""
    return n * np.arange(nchunks + 1, dtype=np.int64) // nchunks


# ------------------------------------------------------------------ what the selection sees of a workspace
def _finish(W):
    W["nchunks"] = plan_of(W["num_local"], W["nb"], W["nrx"], W["ntx"], 1024)["nchunks"]
    for B in W["blocks"]:
        assert (np.diff(B["tx"]) >= 0).all()   # the hit blocks are in TX segments
        B["seg"] = np.searchsorted(B["tx"], np.arange(W["ntx"] + 1))
    return W


def describe(tr):
    """W of tr's last trace (device reads: once per tracer)"""
    counts = tr.counts()
    W = dict(nrx=tr.nrx, ntx=tr.ntx, nb=tr.nb, num_local=tr.num_local, num_paths=tr.num_paths, blocks=[],
             dirs=PL.launch_dirs(tr), counts=counts)
    for b in range(tr.nb):
        n = int(counts[b + 1])
        hb = tr.hit_block(b)
        ray = hb[PL.HIT_RAY, :n].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        tx, path = tr.global_path(ray)
        recs = tr.rec_block(b)[:, PL.REC_DIRX:PL.REC_DIRZ + 1, :n].cpu().numpy().view(np.float32)
        W["blocks"].append(dict(n=n, tx=tx, path=path, tri=hb[HIT_TRI, :n].cpu().numpy().view(np.uint32).copy(),
                                urx=np.ascontiguousarray(recs.transpose(0, 2, 1))))
    L = tr.los()
    W["los"] = []
    for rx in range(tr.nrx):
        for tx in range(tr.ntx):
            q = L[rx, tx]
            st = int(q[0:1].view(np.uint32)[0])
            if st == 1 or tr.shard.rank != 0:
                W["los"].append(None)
            elif st == 2:
                W["los"].append(dict(a=q[1], tau=q[2], nu=q[6], u=q[3:6].astype(np.float64)))
            else:
                W["los"].append(dict(a=np.float32(1), tau=np.float32(0), nu=np.float32(0),
                                     u=np.array([-1.0, 0.0, 0.0])))
    return _finish(W)


def synthetic(case, seed=0):
    """a W as the closed room gives it, without a device: every ray hits in both blocks, each TX segment in a seeded
    order of its rays, made-up triangles and directions, a clear LoS entry per link"""
    c = CASES[case]
    rng = np.random.default_rng(seed)
    n = c["rays"]
    W = dict(nrx=c["nrx"], ntx=c["ntx"], nb=NB, num_local=n, num_paths=n, blocks=[],
             dirs=_units(rng, n).astype(np.float64))
    for b in range(NB):
        ray = np.concatenate([t * n + rng.permutation(n) for t in range(c["ntx"])])
        W["blocks"].append(dict(n=ray.size, tx=ray // n, path=ray % n, tri=rng.integers(0, 12, ray.size).astype(np.uint32),
                                urx=_units(rng, c["nrx"] * ray.size).reshape(c["nrx"], ray.size, 3)))
    W["counts"] = np.array([c["ntx"] * n] * (NB + 1) + [0])
    W["los"] = [dict(a=np.float32(2.0 ** -10 * (1 + l)), tau=np.float32(2.0 ** -24), nu=np.float32(0),
                     u=_units(rng, 1)[0].astype(np.float64)) for l in range(c["nrx"] * c["ntx"])]
    return _finish(W)


def _units(rng, n):
    u = rng.normal(size=(n, 3))
    return (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)


def full_blocks(W):
    """every ray of every TX has a record in both blocks (what the cases are sized for)"""
    return all(int(W["counts"][b + 1]) == W["ntx"] * W["num_local"] for b in range(W["nb"]))


# ------------------------------------------------------------------ the planted values
def _walk(W, tx):
    """of the records of TX segment tx, block by block in index order (the link's visiting positions): block, offset
    in the segment, chunk, and the rank in the order the workgroups walk them (chunk, block, offset)"""
    nch = W["nchunks"]
    blk, off, chunk = [], [], []
    for b, B in enumerate(W["blocks"]):
        n = int(B["seg"][tx + 1] - B["seg"][tx])
        j = np.arange(n)
        blk.append(np.full(n, b))
        off.append(j)
        chunk.append(np.searchsorted(chunk_starts(n, nch), j, side="right") - 1)
    blk, off, chunk = np.concatenate(blk), np.concatenate(off), np.concatenate(chunk)
    order = np.lexsort((off, blk, chunk))
    w = np.empty(order.size, np.int64)
    w[order] = np.arange(order.size)
    return blk, off, chunk, w


def values(W, order, seed=0):
    """v [n] per block: distinct integers 1 .. M within every TX segment (M its records in all blocks), a function of
    the visiting position alone (the same for every receiver)"""
    out = [np.zeros(B["n"], np.int64) for B in W["blocks"]]
    for tx in range(W["ntx"]):
        blk, off, chunk, w = _walk(W, tx)
        M = blk.size
        pos = np.arange(M)
        rng = np.random.default_rng([seed, tx, ORDERS.index(order)])
        if order == "asc":
            v = pos + 1
        elif order == "desc":
            v = M - pos
        elif order == "chunk_asc_record_desc":
            size = np.bincount(chunk, minlength=W["nchunks"])
            base = np.concatenate([[0], np.cumsum(size)])[chunk]
            v = base + size[chunk] - (w - base)
        elif order == "middle_chunk":
            mid = np.nonzero(chunk == W["nchunks"] // 2)[0]
            top = rng.permutation(mid)[:min(1024, mid.size)]
            v = np.zeros(M, np.int64)
            v[top] = M - rng.permutation(top.size)
            rest = np.nonzero(v == 0)[0]
            v[rest] = 1 + rng.permutation(rest.size)
        elif order == "shuffled":
            v = 1 + rng.permutation(M)
        else:
            raise ValueError(order)
        assert np.array_equal(np.sort(v), 1 + pos) and M + 1 < 1 << 24
        for b, B in enumerate(W["blocks"]):
            out[b][B["seg"][tx]:B["seg"][tx + 1]] = v[blk == b]
    return out


def live_bits(W, live):
    """the unblocked bit of every record (a function of its hit index, the same for every receiver)"""
    out = []
    for B in W["blocks"]:
        i = np.arange(B["n"])
        out.append({"all": i >= 0, "odd": i % 2 == 1, "runs": i % RUN_PERIOD < RUN_ON}[live])
    return out


def amplitudes_of(v):
    """[4, n] float32: a_te_re = v, the other three components 0 (power = v^2 exactly in FP64)"""
    a = np.zeros((4, v.size), np.float32)
    a[0] = v
    assert np.array_equal(a[0].astype(np.int64), v)
    return a


def _n_of(b, i):
    return (b << 20) + i + 1   # the planted delay and Doppler of a record are functions of where it is


def terms(W, amps, live):
    """the term list (planted.TERM_KEYS) of W planted with amps [4, n] and live [n] per block, plus "tri" (the row of
    the device table of every term; 0xFFFFFFFF for the LoS entries)"""
    parts, tri = [], []
    for b, B in enumerate(W["blocks"]):
        i = np.nonzero(live[b])[0]
        for rx in range(W["nrx"]):
            t = PL.empty_terms()
            t["rx"], t["tx"], t["bounce"] = np.full(i.size, rx), B["tx"][i], np.full(i.size, b)
            t["index"], t["path"], t["n"] = i, B["path"][i], _n_of(b, i)
            # (the parts set one by one: a sum with 1j times a part loses the sign of a -0.0)
            a = np.ascontiguousarray(amps[b][:, i].T.astype(np.float64))
            t["a_te"], t["a_tm"] = a[:, 0:2].copy().view(np.complex128)[:, 0], a[:, 2:4].copy().view(np.complex128)[:, 0]
            t["tau"] = PL.delay(t["n"]).astype(np.float64)
            t["nu"] = np.asarray(PL.NUS)[t["n"] % 4]
            t["urx"], t["utx"] = B["urx"][rx, i].astype(np.float64), W["dirs"][B["path"][i]]
            t["los"] = np.zeros(i.size, bool)
            parts.append(t)
            tri.append(B["tri"][i])
    for l, q in enumerate(W["los"]):
        if q is None:
            continue
        t = PL.empty_terms()
        t["rx"], t["tx"] = np.array([l // W["ntx"]]), np.array([l % W["ntx"]])
        t["bounce"] = t["index"] = t["path"] = np.array([-1])
        t["n"], t["los"] = np.array([0]), np.array([True])
        t["a_te"] = t["a_tm"] = np.array([complex(q["a"], 0)])
        t["tau"], t["nu"] = np.array([float(q["tau"])]), np.array([float(q["nu"])])
        t["utx"], t["urx"] = q["u"][None, :], -q["u"][None, :]
        parts.append(t)
        tri.append(np.array([0xFFFFFFFF], np.uint32))
    T = PL.concat(PL.empty_terms(), *parts)
    T["tri"] = np.concatenate(tri).astype(np.uint32) if tri else np.zeros(0, np.uint32)
    return T


def order_terms(W, order, live):
    return terms(W, [amplitudes_of(v) for v in values(W, order)], live_bits(W, live))


def plant_records(tr, W, amps, live):
    """Overwrite, for every receiver, every record below the count of every block: the four amplitude fields := amps,
    tau and the Doppler fields := functions of the hit index, the unblocked bits := live (switched ON where the trace
    had them off: such a record's fields are the planted ones too).  The directions stay as traced."""
    torch = tr.torch
    torch.cuda.synchronize(tr.device)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(tr.device)   # noqa: E731
    for b, B in enumerate(W["blocks"]):
        n = B["n"]
        nn = _n_of(b, np.arange(n))
        blk = tr.rec_block(b)
        blk[:, PL.REC_A_TE_RE:PL.REC_A_TM_IM + 1, :n] = dev(amps[b])[None]
        blk[:, PL.REC_TAU, :n] = dev(PL.delay(nn))[None]
        blk[:, PL.REC_DFS, :n] = dev((-np.asarray(PL.NUS)[nn % 4]).astype(np.float32))[None]
        tr.hit_block(b)[PL.HIT_FS0, :n] = 0
        PL._write_mask_bits(tr, b, n, np.broadcast_to(live[b], (tr.nrx, n)))
    torch.cuda.synchronize(tr.device)
    return terms(W, amps, live)


def plant_order(tr, order, live, W=None):
    W = describe(tr) if W is None else W
    return plant_records(tr, W, [amplitudes_of(v) for v in values(W, order)], live_bits(W, live))


# ------------------------------------------------------------------ the reference, with the triangles
def cols_of(T):
    """dominant.reference's columns of a term list, `tri` from T["tri"]"""
    f32 = lambda x: np.asarray(x).astype(np.float32)   # noqa: E731
    a_te, a_tm = T["a_te"].astype(np.complex64), T["a_tm"].astype(np.complex64)
    return dict(power=dominant.term_power(a_te, a_tm), path=T["path"].astype(np.int64).view(U64),
                bounce=T["bounce"].astype(np.int32), tri=T["tri"], a_te=a_te, a_tm=a_tm, tau=f32(T["tau"]),
                freq_shift=f32(T["nu"]), u_rx=f32(T["urx"]), u_tx=f32(T["utx"]))


def reference(T, nrx, ntx, K):
    """dominant.reference(T) with the triangles of T["tri"]"""
    return dominant.from_terms(T["rx"] * ntx + T["tx"], cols_of(T), nrx, ntx, K)


def keys_of(power, bounce, path):
    """hi, lo of the 128-bit key (csrc/hrt_dominant.h)"""
    hi = np.ascontiguousarray(power, np.float64).view(U64) + U64(1)
    path = np.asarray(path).astype(np.int64).view(U64) & U64((1 << PATH_BITS) - 1)
    lo = ~(((np.asarray(bounce).astype(np.int64) + 1).astype(U64) << U64(PATH_BITS)) | path)
    return hi, lo


def chunk_terms(W, T):
    """terms_by_chunk: per link dict(chunks=[per chunk: per block dict(n, off, hi, lo, id)], los=(hi, lo, id) | None)
    with id the term's index in T, off its record's offset from the chunk's start within the block"""
    cols = cols_of(T)
    hi, lo = keys_of(cols["power"], cols["bounce"], cols["path"])
    nch = W["nchunks"]
    link = T["rx"] * W["ntx"] + T["tx"]
    out = []
    for l in range(W["nrx"] * W["ntx"]):
        tx = l % W["ntx"]
        mine = np.nonzero(link == l)[0]
        los = mine[T["los"][mine]]
        chunks = [[] for _ in range(nch)]
        for b, B in enumerate(W["blocks"]):
            s0, n = int(B["seg"][tx]), int(B["seg"][tx + 1] - B["seg"][tx])
            starts = chunk_starts(n, nch)
            ids = mine[(T["bounce"][mine] == b) & ~T["los"][mine]]
            j = T["index"][ids] - s0
            assert (np.diff(j) > 0).all() and (j.size == 0 or (j[0] >= 0 and j[-1] < n))
            cut = np.searchsorted(j, starts)
            for c in range(nch):
                s = ids[cut[c]:cut[c + 1]]
                chunks[c].append(dict(n=int(starts[c + 1] - starts[c]), off=j[cut[c]:cut[c + 1]] - starts[c],
                                      hi=hi[s], lo=lo[s], id=s, start=s0 + int(starts[c])))
        out.append(dict(chunks=chunks, los=(hi[los], lo[los], los) if los.size else None))
    return out


# ------------------------------------------------------------------ the model of the three kernels
class _Slots:
    """the LDS of one workgroup: the kept candidates (sorted, at most K), the pending ones, the threshold"""

    def __init__(self, K, wrong, st):
        self.K, self.wrong, self.st = K, wrong, st
        self.kept = (np.zeros(0, U64), np.zeros(0, U64), np.zeros(0, np.int64))
        self.pend = []
        self.c = 0
        self.th, self.tl = U64(0), U64(0)
        self.flushes = self.kept_flushes = 0

    def room(self, need):
        lim = N - self.K
        if self.wrong == "room_ge":
            full = self.c + need >= lim
        elif self.wrong == "room_late":
            full = self.c > lim
        else:
            full = self.c + need > lim
        if full:
            self.flush()

    def push(self, hi, lo, ix):
        """the candidates of one step, as they are (no threshold)"""
        left = N - self.K - self.c
        if hi.size > left:   # past slot N: lost (only a wrong dm_room gets here)
            assert self.wrong == "room_late", (hi.size, left)
            hi, lo, ix = hi[:left], lo[:left], ix[:left]
        if hi.size:
            self.pend.append((hi, lo, ix))
            self.c += hi.size
            self.st["pushed"] += hi.size
        self.st["max_pending"] = max(self.st["max_pending"], self.c)
        if self.c == N - self.K and hi.size:
            self.st["exact"] += 1

    def offer(self, hi, lo, ix):
        """the candidates of one step that beat the threshold"""
        if self.wrong == "thr_ge":
            ok = hi >= self.th
        elif self.wrong == "thr_gt_hi":
            ok = hi > self.th
        else:
            ok = (hi > self.th) | ((hi == self.th) & (lo > self.tl))
        self.push(hi[ok], lo[ok], ix[ok])

    def flush(self):
        K = self.K
        hi, lo, ix = (np.concatenate([self.kept[q]] + [p[q] for p in self.pend]) for q in range(3))
        if self.wrong == "hi_only_sort":
            order = np.argsort(hi, kind="stable")[::-1]
        else:
            order = np.lexsort((lo, hi))[::-1]
        order = order[:K]
        self.flushes += 1
        self.kept_flushes += bool((order >= self.kept[0].size).any())
        self.kept = (hi[order], lo[order], ix[order])
        self.pend, self.c = [], 0
        self.th, self.tl = (hi[order[-1]], lo[order[-1]]) if order.size == K else (U64(0), U64(0))

    def done(self):
        self.flush()
        self.st["flushes"] += self.flushes
        self.st["kept_flushes"].append(self.kept_flushes)
        return self.kept


def _stream(S, lists, step):
    """dm_stream over lists of K slots each (a list's empty slots are at its end and are skipped)"""
    K = S.K
    total = len(lists) * K
    hi, lo, ix = (np.concatenate([l[q] for l in lists]) if lists else np.zeros(0, U64) for q in range(3))
    slot = np.concatenate([i * K + np.arange(l[0].size) for i, l in enumerate(lists)]) if lists else np.zeros(0, int)
    for base in range(0, total, step):
        S.room(step)
        s = slice(*np.searchsorted(slot, (base, base + step)))
        S.offer(hi[s], lo[s], ix[s])


def _stats():
    return {k: dict(max_pending=0, exact=0, flushes=0, kept_flushes=[], pushed=0) for k in ("partial", "merge", "final")}


def old_rows(old, l):
    """the keys of the records the output holds for link l (id: -1 - slot), kept not clamped"""
    nrx, ntx, K = old["power"].shape
    rx, tx = divmod(l, ntx)
    kept = int(old["kept"][rx, tx])
    hi, lo = keys_of(old["power"][rx, tx], old["bounce"][rx, tx], old["path"][rx, tx])
    return kept, hi, lo, -1 - np.arange(K)


def model(tbc, K, nrx, ntx, cols, old=None, wrong=None, other=None):
    """The selection of csrc/hrt_dominant.hip on terms_by_chunk (chunk_terms): the result dict (dominant.from_terms'
    layout, the records gathered from cols, or from `old` when accumulating) and the counters per kernel: the largest
    pending count, the steps that ended with the pending slots exactly full (N - K), the flushes, per workgroup the
    flushes that kept a pending candidate, the candidates pushed; and `single` (merge groups of one list) and `empty` (empty lists read).
    other: for wrong="merge_unclamped", which link's lists lie behind a link's in the scratch."""
    st = _stats()
    st["single"] = st["empty"] = 0
    out = dominant.empty(nrx, ntx, K)
    nl = nrx * ntx
    la, ca = [], []
    for L in tbc:
        lists, counts = [], []
        for chunk in L["chunks"]:
            S = _Slots(K, wrong, st["partial"])
            for B in chunk:
                step = B["off"] // PARTIAL_STEP
                cut = np.searchsorted(step, np.arange(-(-B["n"] // PARTIAL_STEP) + 1))
                for k in range(cut.size - 1):
                    S.room(PARTIAL_STEP)
                    s = slice(cut[k], cut[k + 1])
                    S.offer(B["hi"][s], B["lo"][s], B["id"][s])
            lists.append(S.done())
            counts.append(sum(B["off"].size for B in chunk))
        la.append(lists)
        ca.append(counts)
    for l, L in enumerate(tbc):
        nch = len(L["chunks"])
        nmid = -(-nch // FANIN) if nch > FANIN else 0
        lists, counts = la[l], ca[l]
        if nmid:
            lb, cb = [], []
            for m in range(nmid):
                l0 = m * FANIN
                l1 = min(l0 + FANIN, nch)
                src = la[l][l0:l1]
                if wrong == "merge_skips_last":
                    src = la[l][l0:min(l0 + FANIN - 1, nch)]
                elif wrong == "merge_unclamped" and l0 + FANIN > nch and other is not None:
                    src = src + la[other[l]][:l0 + FANIN - nch]
                st["single"] += len(src) == 1
                st["empty"] += sum(s[0].size == 0 for s in src)
                S = _Slots(K, wrong, st["merge"])
                _stream(S, src, MERGE_STEP)
                lb.append(S.done())
                cb.append(ca[l][l0] if wrong == "count_not_summed" else sum(ca[l][l0:l1]))
            lists, counts = lb, cb
            if wrong == "final_reads_la":
                lists, counts = la[l][:nmid], ca[l][:nmid]
        S = _Slots(K, wrong, st["final"])
        eligible = 0
        if old is not None:
            kept_old, hi, lo, ix = old_rows(old, l)
            eligible = int(old["eligible"][l // ntx, l % ntx])
            if wrong != "kept_unclamped":
                kept_old = min(kept_old, K)
            S.push(hi[:kept_old], lo[:kept_old], ix[:kept_old])
            S.flush()
        if L["los"] is not None:
            eligible += 1
            S.push(*L["los"])
        st["empty"] += sum(s[0].size == 0 for s in lists)
        _stream(S, lists, FINAL_STEP)
        ix = S.done()[2]
        eligible += sum(counts)
        rx, tx = divmod(l, ntx)
        out["kept"][rx, tx], out["eligible"][rx, tx] = ix.size, eligible
        new = ix >= 0
        for k in dominant.FIELDS:
            v = out[k][rx, tx]
            v[np.nonzero(new)[0]] = cols[k][ix[new]]
            if old is None:
                continue
            o = old[k][rx, tx].copy()
            if wrong == "old_in_place":   # slot s is stored before the slots behind it are read
                for s in np.nonzero(~new)[0]:
                    o[:s] = v[:s]
                    v[s] = o[-1 - ix[s]]
            else:
                v[np.nonzero(~new)[0]] = o[-1 - ix[~new]]
    assert out["kept"].size == nl
    return out, st


def run_model(W, T, K, **kw):
    return model(chunk_terms(W, T), K, W["nrx"], W["ntx"], cols_of(T), **kw)


def same_bytes(a, b):
    return np.array_equal(a["buffer"], b["buffer"])


# ------------------------------------------------------------------ which edges a combination reaches
def features(W, T, K, st=None):
    """the edges a (case, order, live, K) reaches, as (name, value) pairs: what SURVIVORS is chosen by"""
    if st is None:
        st = run_model(W, T, K)[1]
    f = []
    for k in ("partial", "merge", "final"):
        s = st[k]
        f.append((k + "_exact", s["exact"] > 0))
        f.append((k + "_full", s["max_pending"] == N - K))
        f.append((k + "_flushes", min(max(s["kept_flushes"], default=0), 3)))
        f.append((k + "_idle_flush", any(n == 1 for n in s["kept_flushes"]) and s["flushes"] > len(s["kept_flushes"])))
    f.append(("single", st["single"] > 0))
    f.append(("split_word", starts_inside_word(W, T)))
    f.append(("short", int(np.bincount(T["rx"] * W["ntx"] + T["tx"]).min()) < K))
    return f


def starts_inside_word(W, T):
    """a chunk starts inside a mask word, and that word and the next hold bits of both kinds"""
    live = np.zeros((W["nb"], max(B["n"] for B in W["blocks"]) + 64), bool)
    s = ~T["los"] & (T["rx"] == 0)
    live[T["bounce"][s], T["index"][s]] = True
    for b, B in enumerate(W["blocks"]):
        for tx in range(W["ntx"]):
            s0, n = int(B["seg"][tx]), int(B["seg"][tx + 1] - B["seg"][tx])
            for start in s0 + chunk_starts(n, W["nchunks"])[:-1]:
                w0 = start // 64 * 64
                word = live[b, w0:min(w0 + 128, B["n"])]
                if start % 64 and word.any() and not word.all():
                    return True
    return False


def derive(case, W=None, check=None):
    """the combinations of a case that survive (see SURVIVORS), and the features and counters of every combination;
    check(order, live, K, T, result) sees every result of the model"""
    W = synthetic(case) if W is None else W
    seen, keep, feats = set(), [], {}
    for order, live in combos(case):
        T = order_terms(W, order, live)
        tbc, cols = chunk_terms(W, T), cols_of(T)
        for K in CASES[case]["ks"][::-1]:
            got, st = model(tbc, K, W["nrx"], W["ntx"], cols)
            if check is not None:
                check(order, live, K, T, got)
            f = set(features(W, T, K, st)) | {("order", (order, live)), ("K", K)}
            feats[(order, live, K)] = (f, st)
            if f - seen or (case, order, live, K) in NAMED:
                keep.append((case, order, live, K))
            seen |= f
    return keep, feats


# The combinations the GPU file runs: per case, in the order of combos() x the case's K values from the largest down,
# every combination whose features() hold a (name, value) that no earlier one of the case has (so every order and live
# pattern runs at the largest K at least, and every K once), and the ones the design test names.
# tests/test_dominant_order_design.py derives this list again and compares.
NAMED = (
    ("cap_1024", "asc", "all", 1024), ("cap_1536", "asc", "all", 512), ("merge_two_full", "asc", "all", 1024),
    ("fanin_full", "asc", "all", 1024), ("merge_tail_one", "asc", "all", 1024), ("cap_1024", "desc", "all", 1024),
    ("fanin_full", "asc", "odd", 513), ("merge_tail_one", "shuffled", "runs", 1023),
    ("two_by_two", "asc", "all", 1024), ("two_by_two", "shuffled", "runs", 512),
)
_ASC = ("asc", "all", KS_ALL[::-1])
_ONCE = tuple((o, l, (1024,)) for o, l in (("chunk_asc_record_desc", "all"), ("middle_chunk", "all"),
                                           ("shuffled", "all"), ("asc", "odd"), ("asc", "runs"), ("shuffled", "odd"),
                                           ("shuffled", "runs")))
_DESC = ("desc", "all", (1024, 1023, 513))
_BIG = (("asc", "all", (1024, 1023, 512)), ("desc", "all", (1024, 1023)), ("chunk_asc_record_desc", "all", (1024,)),
        ("shuffled", "all", (1024,)), ("asc", "runs", (1024,)))
_KEPT = {
    "one_chunk": (_ASC, ("desc", "all", (1024, 513))) + _ONCE,
    "fanin_full": (_ASC, _DESC) + _ONCE[:3] + (("asc", "odd", (1024, 513)),) + _ONCE[4:],
    "merge_tail_one": (_ASC, _DESC) + _ONCE[:6] + (("shuffled", "runs", (1024, 1023)),),
    "merge_two_full": (_ASC, _DESC) + _ONCE,
    "cap_1024": _BIG,
    "cap_1536": _BIG,
    "two_by_two": (_ASC, _DESC) + _ONCE[:6] + (("shuffled", "runs", (1024, 512)),),
}
# the kernels whose pending slots a combination fills exactly to N - K (asserted from the model: in the design test
# on full blocks, in the GPU file on the segments the trace left)
EXACT_FILL = {
    ("cap_1024", "asc", "all", 1024): ("partial", "merge", "final"),
    ("cap_1536", "asc", "all", 512): ("partial",),
    ("merge_two_full", "asc", "all", 1024): ("merge",),
    ("fanin_full", "asc", "all", 1024): ("final",),
}
LOST_MAX = 16   # rays per block the room may lose (a ray that meets an edge of the room exactly)
SURVIVORS = tuple((case, o, l, K) for case in CASES for o, l, ks in _KEPT[case] for K in ks)


# ------------------------------------------------------------------ equal powers, extreme powers, a chosen `out`
def equal_amplitudes(W):
    """every record (3, 4 | 0, 0): power 25 everywhere, the order is (bounce, path) alone"""
    out = []
    for B in W["blocks"]:
        a = np.zeros((4, B["n"]), np.float32)
        a[0], a[1] = 3, 4
        out.append(a)
    return out


EXTREME_K = 64
# (block, hit index, the four amplitude components); everything else is blocked
EXTREMES = (
    (0, 0, (0.0, 0.0, 0.0, 0.0)), (0, 63, (-0.0, 0.0, -0.0, 0.0)), (1, 64, (-0.0, -0.0, -0.0, -0.0)),
    (0, 65, (1e-45, 0.0, 0.0, 0.0)), (1, 127, (0.0, 0.0, -1e-45, 0.0)),
    (0, 300, (3e38, 3e38, 3e38, 3e38)), (1, 599, (-3e38, 3e38, -3e38, 3e38)),
    (1, 5, (3.0, 4.0, 0.0, 0.0)), (0, 511, (5.0, 0.0, 0.0, 0.0)), (0, 512, (0.0, 0.0, 0.0, 5.0)),
    (1, 513, (0.0, -5.0, 0.0, 0.0)), (0, 7, (1.0, 0.0, 0.0, 0.0)),
)


def extreme_records(W):
    """amps, live of W planted with EXTREMES alone"""
    amps = [np.zeros((4, B["n"]), np.float32) for B in W["blocks"]]
    live = [np.zeros(B["n"], bool) for B in W["blocks"]]
    for b, i, a in EXTREMES:
        amps[b][:, i] = np.array(a, np.float32)
        live[b][i] = True
    return amps, live


OLD_KINDS = ("stronger", "weaker", "even", "half")
OLD_BOUNCE = 7   # no planted record has it (the traces have two bounces)


def old_list(T, K, kind, nrx, ntx):
    """A result a call accumulates into, of records no term of T is (bounce OLD_BOUNCE, path 1000 + s): per link K
    records stronger than every term of T, weaker than every one, at ranks 2, 4, 6 ... of the union counted from 1
    (`even`: old record s would move to slot 2 s + 1), or the first K / 2 (at least one) of the latter (`half`)."""
    power = cols_of(T)["power"]
    link = T["rx"] * ntx + T["tx"]
    links, cols = [], {k: [] for k in dominant.FIELDS}
    for l in range(nrx * ntx):
        p = np.sort(power[link == l])[::-1]
        assert p.size > K + 1 and p[-1] > 0
        n = max(K // 2, 1) if kind == "half" else K
        s = np.arange(n)
        if kind == "stronger":
            q = p[0] + (K - s).astype(np.float64)
        elif kind == "weaker":
            q = p[-1] / (s + 2)
        else:
            q = ((np.sqrt(p[s]) + np.sqrt(p[s + 1])) / 2) ** 2
            assert (q < p[s]).all() and (q > p[s + 1]).all()
        links.append(np.full(n, l))
        cols["power"].append(q)
        cols["path"].append((1000 + s).astype(U64))
        cols["bounce"].append(np.full(n, OLD_BOUNCE, np.int32))
        cols["tri"].append((77 + s).astype(np.uint32))
        cols["a_te"].append(np.sqrt(q).astype(np.complex64))
        cols["a_tm"].append(np.zeros(n, np.complex64))
        cols["tau"].append((s * 2.0 ** -20).astype(np.float32))
        cols["freq_shift"].append(s.astype(np.float32))
        cols["u_rx"].append(np.tile(np.array([1, 0, 0], np.float32), (n, 1)))
        cols["u_tx"].append(np.tile(np.array([0, 1, 0], np.float32), (n, 1)))
    old = dominant.from_terms(np.concatenate(links), {k: np.concatenate(v) for k, v in cols.items()}, nrx, ntx, K)
    old["eligible"][...] += 1000 * (1 + np.arange(nrx * ntx, dtype=np.uint64).reshape(nrx, ntx))
    return old


def old_slots(res, old):
    """per link, the slot of `res` every record of `old` stands in (-1: not kept)"""
    nrx, ntx, K = old["power"].shape
    out = np.full((nrx, ntx, K), -1)
    for rx in range(nrx):
        for tx in range(ntx):
            kept = int(res["kept"][rx, tx])
            mine = np.nonzero(res["bounce"][rx, tx, :kept] == OLD_BOUNCE)[0]
            out[rx, tx, res["path"][rx, tx, mine].astype(np.int64) - 1000] = mine
    return out
