"""hrt_apply_patterns record by record, on planted workspaces (tests/planted.py, tests/patterns_util.py).

After a real trace the test writes the amplitudes itself: they are in {1, 2} j^k (TM: half of it), so each field after
the apply step is +-w, +-2w or +-w/2 exactly and the test reads w bit for bit (patterns_util.check_applied).  Every
check compares the whole workspace before and after: the live amplitudes carry the weight of the definition, and no
other byte has changed.

Shapes: C1 (one link, one block of 3000 hits) and the two-TX C4 at 3000 rays per TX (2469, 22 and 2 hits, then three
empty blocks: counts that are no multiple of 64, several workgroups, an empty block), with two and with four receivers.
Tolerance: patterns_util.weight_tolerance (4 x the float32 floor per side); exact cases at 0."""
import ctypes as C

import numpy as np
import pytest

from hermespy_rt_amd import abi
from hermespy_rt_amd import patterns as P

from . import configs as K
from . import patterns_util as U
from . import planted as PL
from .pathsum_util import _force_los_classes, _tracer

pytestmark = pytest.mark.gpu

RAYS = 3000
CONFIGS = {"C1": lambda: K.small(K.C1, RAYS), "C4": lambda: K.small(K.C4, RAYS), "C4_RX4": lambda: U.c4_rx4(RAYS)}


class Planted:
    def __init__(self, name, **kw):
        self.name = name
        self.tr = _tracer(CONFIGS[name](), **kw)
        self.tr.trace()
        self.T = PL.plant(self.tr, keyed=True)
        self.counts = self.tr.counts()
        self.before = U.snapshot(self.tr)

    def run(self, rx=None, tx=None, R_rx=None, R_tx=None, before=None):
        U.restore(self.tr, self.before if before is None else before)
        return U.apply(self.tr, rx, tx, R_rx, R_tx)


@pytest.fixture(scope="module")
def planted():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Planted(name)
        return made[name]

    yield get
    for p in made.values():
        p.tr.close()


def _orient(p, seed=0):
    return U.random_rotations(p.tr.nrx, 100 + seed), U.random_rotations(p.tr.ntx, 200 + seed)


def test_shapes_are_the_ones_the_module_names(planted):
    c = planted("C4").counts
    assert [int(x) for x in c[1:7]] == [2469, 22, 2, 0, 0, 0] and planted("C4").tr.cap == 6144
    assert int(planted("C1").counts[1]) == 3000 and planted("C1").tr.nrx == 1
    assert planted("C4_RX4").tr.nrx == 4 and planted("C4_RX4").tr.ntx == 2
    for name in CONFIGS:
        p = planted(name)
        assert (~p.T["los"]).sum() > 500 and (PL.los_status(p.tr) == 2).any(), name


# ------------------------------------------------------------------ exact cases, at tolerance 0
@pytest.mark.parametrize("name", ["C1", "C4"])
def test_isotropic_leaves_every_byte(planted, name):
    p = planted(name)
    R_rx, R_tx = _orient(p)
    for kw in (dict(rx=P.isotropic(), tx=P.isotropic()), dict(rx=P.isotropic(), R_rx=R_rx, R_tx=R_tx),
               dict(rx=P.table(np.ones((2, 1))), tx=P.table(np.ones((181, 360))), R_rx=R_rx)):
        after = p.run(**kw)
        assert np.array_equal(after, p.before), kw


@pytest.mark.parametrize("name", ["C1", "C4", "C4_RX4"])
def test_constant_tables_scale_by_exactly_one_sixteenth(planted, name):
    p = planted(name)
    R_rx, R_tx = _orient(p, 1)
    rx, tx = P.table(np.full((181, 360), 0.5, np.float32)), P.table(np.full((7, 5), 2.0 ** -3, np.float32))
    after = p.run(rx, tx, R_rx, R_tx)
    U.check_applied(p.tr, p.before, after, p.T, rx, tx, R_rx, R_tx, exact=2.0 ** -4, what=name)
    # gains are factors too: +6.0206 dB is not a power of two, -200 .. 200 dB stay finite
    rx = P.table(np.full((2, 1), 0.5, np.float32), gain_db=20.0)
    r = U.check_applied(p.tr, p.before, p.run(rx, tx, R_rx, R_tx), p.T, rx, tx, R_rx, R_tx, what=name)
    assert np.all(r["w"] == np.float32(10.0) * np.float32(0.5) * np.float32(0.125))


def test_zero_table_zeroes_the_live_amplitudes_and_nothing_else(planted):
    p = planted("C4")
    rx, tx = P.table(np.zeros((3, 4), np.float32)), P.tr38901()
    after = p.run(rx, tx, None, None)
    r = U.check_applied(p.tr, p.before, after, p.T, rx, tx, None, None, exact=0.0, what="zero table")
    assert r["w"].size == np.unique(np.stack([p.T["rx"], p.T["bounce"], p.T["index"]], 1)[~p.T["los"]], axis=0).shape[0] \
        + r["clear"].size


def test_two_runs_give_the_same_bytes(planted):
    p = planted("C4_RX4")
    R_rx, R_tx = _orient(p, 2)
    pats = U.pattern_set()
    a = p.run(pats["table_181x360"], pats["tr38901"], R_rx, R_tx)
    b = p.run(pats["table_181x360"], pats["tr38901"], R_rx, R_tx)
    assert np.array_equal(a, b) and not np.array_equal(a, p.before)


# ------------------------------------------------------------------ per-record comparison against weight()
@pytest.mark.parametrize("side", ["rx", "tx"])
@pytest.mark.parametrize("kind", list(U.pattern_set()))
def test_weights_of_every_kind_on_each_side(planted, kind, side):
    pats = U.pattern_set()
    other = pats["dipole"] if side == "rx" else pats["tr38901"]
    rx, tx = (pats[kind], other) if side == "rx" else (other, pats[kind])
    for name, seed in (("C4", 3), ("C1", 4)):
        p = planted(name)
        R_rx, R_tx = _orient(p, seed)
        r = U.check_applied(p.tr, p.before, p.run(rx, tx, R_rx, R_tx), p.T, rx, tx, R_rx, R_tx, what="%s %s %s" % (name, side, kind))
        print(name, side, kind, "weights", r["w"].size, "largest |w - ref| / tol", r["ratio"])
        assert r["w"].min() >= 0 and len(np.unique(r["w"])) > (1 if kind == "isotropic" else 10)


def test_receivers_and_transmitters_have_their_own_orientation(planted):
    """nrx = 4 and ntx = 2 with different orientations: the RX weight follows the record's receiver, the TX weight
    the transmitter of HRT_HIT_RAY; with one endpoint's orientation for all of its side the comparison fails"""
    p = planted("C4_RX4")
    R_rx, R_tx = _orient(p, 5)
    rx, tx = P.tr38901(), P.tr38901(3.0)
    after = p.run(rx, tx, R_rx, R_tx)
    U.check_applied(p.tr, p.before, after, p.T, rx, tx, R_rx, R_tx, what="own orientations")
    for wrong in (dict(R_tx=R_tx[:1].repeat(2, axis=0)), dict(R_tx=R_tx[::-1].copy()), dict(R_rx=R_rx[[1, 0, 3, 2]]),
                  dict(R_rx=R_rx[:1].repeat(4, axis=0))):
        with pytest.raises(AssertionError):
            U.check_applied(p.tr, p.before, after, p.T, rx, tx, **dict(dict(R_rx=R_rx, R_tx=R_tx), **wrong))
    # one (3, 3) orientation serves every endpoint of the side
    after = p.run(rx, tx, R_rx[2], R_tx[1])
    U.check_applied(p.tr, p.before, after, p.T, rx, tx, R_rx[2:3].repeat(4, axis=0), R_tx[1:].repeat(2, axis=0))


def _replant_special(p):
    """the directions of the live records (RX side) and of the clear LoS entries (TX side; RX = its negative) on the
    poles, the axes and the +-180 degree seam of the local frames: exact rotations, u = R^T d"""
    tr = p.tr
    Rs, d = U.exact_rotations(), U.special_local().astype(np.float64)
    R_rx, R_tx = Rs[3:3 + tr.nrx * 5:5].copy(), Rs[7:7 + tr.ntx * 4:4].copy()
    U.restore(tr, p.before)
    T = {k: v.copy() for k, v in p.T.items()}
    s = np.nonzero(~T["los"])[0]
    for b in np.unique(T["bounce"][s]):
        blk = tr.rec_block(int(b)).view(tr.torch.float32)
        for rx in range(tr.nrx):
            k = s[(T["bounce"][s] == b) & (T["rx"][s] == rx)]
            u = d[(T["index"][k] + 3 * rx) % d.shape[0]] @ R_rx[rx].astype(np.float64)   # R^T d
            T["urx"][k] = u
            i = tr.torch.from_numpy(T["index"][k]).to(tr.device)
            for c in range(3):
                blk[rx, PL.REC_DIRX + c, i] = tr.torch.from_numpy(u[:, c].astype(np.float32)).to(tr.device)
    L = PL.los_view(tr)
    st = PL.los_status(tr)
    n = 0
    for rx in range(tr.nrx):
        for tx in range(tr.ntx):
            if st[rx, tx] == 2:
                u = d[(5 * n + 1) % d.shape[0]] @ R_tx[tx].astype(np.float64)
                L[rx, tx, PL.LOS_DIRX:PL.LOS_DIRZ + 1] = tr.torch.from_numpy(u.astype(np.float32)).to(tr.device)
                n += 1
    assert n > 0
    return T, R_rx, R_tx, U.snapshot(tr)


@pytest.mark.parametrize("name", ["C4", "C4_RX4"])
def test_directions_on_the_poles_the_axes_and_the_seam(planted, name):
    p = planted(name)
    T, R_rx, R_tx, before = _replant_special(p)
    pats = U.pattern_set()
    for kind, pat in pats.items():
        for rx, tx in ((pat, pats["isotropic"]), (pats["isotropic"], pat), (pat, pat)):
            after = p.run(rx, tx, R_rx, R_tx, before=before)
            r = U.check_applied(p.tr, before, after, T, rx, tx, R_rx, R_tx, what="special %s %s" % (name, kind))
        print(name, kind, "largest |w - ref| / tol", r["ratio"])
    # identity orientations are NULL pointers in the kernel: the same directions, read in the world frame
    after = p.run(pats["table_7x12"], pats["dipole"], None, None, before=before)
    U.check_applied(p.tr, before, after, T, pats["table_7x12"], pats["dipole"], None, None, what="identity")


# ------------------------------------------------------------------ poison
@pytest.mark.parametrize("value", [float("nan"), 1e30])
def test_poison_is_neither_read_nor_written(planted, value):
    p = planted("C4_RX4")
    tr = p.tr
    U.restore(tr, p.before)
    _force_los_classes(tr)
    hit = PL.poison(tr, p.counts, value)
    for cls in ("blocked_records", "tail_slots", "tail_mask_bits", "los_blocked", "los_coincident"):
        assert hit[cls] > 0, (cls, hit)
    before = U.snapshot(tr)
    R_rx, R_tx = _orient(p, 6)
    pats = U.pattern_set()
    for rx, tx in ((pats["tr38901"], pats["table_181x360"]), (pats["dipole"], pats["table_2x3"])):
        after = p.run(rx, tx, R_rx, R_tx, before=before)
        r = U.check_applied(tr, before, after, p.T, rx, tx, R_rx, R_tx, what="poison %r" % value)
        assert np.isfinite(r["w"]).all() and r["clear"].size < tr.nrx * tr.ntx


# ------------------------------------------------------------------ shards
@pytest.mark.parametrize("world", [2, 3])
def test_shards_weight_a_global_path_as_the_whole_does(planted, world):
    whole = planted("C4")
    R_rx, R_tx = _orient(whole, 7)
    pats = U.pattern_set()
    rx, tx = pats["tr38901"], pats["table_7x12"]
    r = U.check_applied(whole.tr, whole.before, whole.run(rx, tx, R_rx, R_tx), whole.T, rx, tx, R_rx, R_tx)
    T = whole.T
    s = np.nonzero(~T["los"])[0][r["terms"]]
    ref = {(int(T["rx"][k]), int(T["tx"][k]), int(T["path"][k]), int(T["bounce"][k])): w
           for k, w in zip(s, r["w"][:s.size])}
    seen = 0
    for rank in range(world):
        sh = Planted("C4", rank=rank, world=world, chunk=64)
        g = U.check_applied(sh.tr, sh.before, sh.run(rx, tx, R_rx, R_tx), sh.T, rx, tx, R_rx, R_tx, what="shard %d" % rank)
        t = np.nonzero(~sh.T["los"])[0][g["terms"]]
        for k, w in zip(t, g["w"][:t.size]):
            key = (int(sh.T["rx"][k]), int(sh.T["tx"][k]), int(sh.T["path"][k]), int(sh.T["bounce"][k]))
            assert ref[key] == w, (key, ref[key], w)   # to the bit
        seen += t.size
        # every shard's LoS entries are weighted as the whole's
        assert np.array_equal(g["w"][t.size:], r["w"][s.size:])
        sh.tr.close()
    assert seen == s.size


# ------------------------------------------------------------------ the physical sense of the directions
def test_a_boresight_at_the_other_endpoint_gives_the_los_its_maximum():
    c = K.small(K.C1, RAYS)
    tr = _tracer(c)
    tr.trace()
    a0 = tr.los()[0, 0].copy()
    assert int(a0[0:1].view(np.uint32)[0]) == 2 and a0[PL.LOS_A] > 0
    rx_pos, tx_pos = np.array(c["rx_pos"][0], np.float64), np.array(c["tx_pos"][0], np.float64)
    g = 10.0 ** (2.0 / 20.0)
    for side in ("tx", "rx"):
        toward = rx_pos - tx_pos if side == "tx" else tx_pos - rx_pos
        for R, db in ((P.look_at(toward), 8.0), (P.look_at(-toward), -22.0)):
            tr.set_patterns(**{side: P.tr38901(2.0), side + "_orientation": R})
            tr.trace()
            assert tr.patterned
            a = tr.los()[0, 0]
            want = float(a0[PL.LOS_A]) * g * 10.0 ** (db / 20.0)
            assert abs(float(a[PL.LOS_A]) - want) <= (2 * U.TOL + 2.0 ** -22) * want, (side, db, a[PL.LOS_A], want)
            assert np.array_equal(a[[0, 2, 3, 4, 5, 6]], a0[[0, 2, 3, 4, 5, 6]])
        tr.set_patterns()
    tr.trace()
    assert not tr.patterned and np.array_equal(tr.los()[0, 0], a0)
    tr.close()


# ------------------------------------------------------------------ negative controls
def test_the_planted_checks_fail_for_one_wrong_record(planted):
    p = planted("C4_RX4")
    R_rx, R_tx = _orient(p, 8)
    rx, tx = P.tr38901(), P.dipole()
    after = p.run(rx, tx, R_rx, R_tx)
    T = p.T
    U.check_applied(p.tr, p.before, after, T, rx, tx, R_rx, R_tx)
    for name, k in PL.control_records(T):
        for how in ("drop", "double"):
            with pytest.raises(AssertionError):
                U.check_applied(p.tr, p.before, after, PL.mutate(T, k, how), rx, tx, R_rx, R_tx)
        swapped = {key: v.copy() for key, v in T.items()}
        swapped["rx"][k] = (T["rx"][k] + 1) % p.tr.nrx
        with pytest.raises(AssertionError):
            U.check_applied(p.tr, p.before, after, swapped, rx, tx, R_rx, R_tx)
    # and an exact check fails for a weight that is one ulp off
    rx, tx = P.table(np.full((2, 1), 0.5, np.float32)), P.table(np.full((2, 1), 0.125, np.float32))
    after = p.run(rx, tx, R_rx, R_tx)
    with pytest.raises(AssertionError):
        U.check_applied(p.tr, p.before, after, T, rx, tx, R_rx, R_tx, exact=float(np.nextafter(np.float32(2.0 ** -4), np.float32(1))))


# ------------------------------------------------------------------ the entries' own rules
def test_refusals_that_need_a_problem_and_the_tracer_members(planted):
    p = planted("C1")
    tr = p.tr
    U.restore(tr, p.before)
    spec = abi.PatternSpec(abi.pattern_struct(P.dipole()), abi.pattern_struct(P.isotropic()), None, None)
    rc = tr.L.hrt_apply_patterns(tr.problem, C.byref(tr.shard), C.c_void_p(tr.ws.data_ptr()),
                                 C.c_uint64(tr.ws.numel() - 1), C.byref(spec), None)
    assert rc == -1 and b"hrt_apply_patterns: workspace of" in tr.L.hrt_last_error()
    tr.torch.cuda.synchronize(tr.device)
    assert np.array_equal(U.snapshot(tr), p.before)
    for kw, what in ((dict(rx_orientation=1.001 * np.eye(3)), "orthonormal"), (dict(tx_orientation=np.eye(4)), "shape"),
                     (dict(rx_orientation=np.stack([np.eye(3)] * 2)), "shape"),
                     (dict(rx=dict(kind=3, gain_db=0.0, table=-np.ones((2, 2)))), "finite and >= 0"),
                     (dict(tx=dict(kind=9, gain_db=0.0)), "kind"), (dict(tx=P.dipole(201.0)), "gain_db")):
        with pytest.raises(ValueError, match=what):
            tr.set_patterns(**kw)
    tr.set_patterns()
    with pytest.raises(RuntimeError, match="no patterns"):
        tr.apply_patterns()
    tr.set_patterns(rx=P.dipole())
    tr.patterned = False
    tr.apply_patterns()
    assert tr.patterned
    with pytest.raises(RuntimeError, match="already weighted"):
        tr.apply_patterns()
    tr.set_patterns()
