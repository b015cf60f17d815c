"""oracle.closest_hits / shadow_dirs / mirror (oracle/hrt_oracle.c): the per-ray exports of the restatement's own
closest_hit that tests/test_gpu_candidates.py uses as its reference.  No GPU."""
import numpy as np
import pytest

from oracle import oracle

from . import configs as K
from . import scenes_gen as G

NO_HIT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def run():
    c = K.small(K.C3, 256)
    return c, oracle.compute_paths(*K.args(c)), oracle.compute_paths_subset(*K.args(c), subset=(0, 256, 1))


def _states(c, ref, b):
    """(o, d) of every ray entering bounce b, from the run's snapshots (one TX: rows b np + p)"""
    n = c["num_paths"]
    s = ref["scat_rays"][b * n:(b + 1) * n]
    return s[:, :3], s[:, 3:]


def test_full_scan_of_reported_states_reproduces_the_hits(run):
    c, ref, sub = run
    assert len(c["tx_pos"]) == 1
    flat = oracle.flatten(oracle.read_hrt(c["scene_path"]))
    total = 0
    for b in range(c["num_bounces"]):
        o, d = _states(c, ref, b)
        tri, dist = oracle.closest_hits(flat, o, d)
        # a ray that missed before keeps its state, so the scan misses again: NO_HIT in both
        assert np.array_equal(tri, ref["extras"]["hit_tri"][b, 0]), "bounce %d" % b
        assert np.array_equal(tri, sub["hit_tri"][b, 0]), "bounce %d (subset run)" % b
        assert np.array_equal(dist[tri == NO_HIT], np.full((tri == NO_HIT).sum(), np.float32(1e9).view(np.uint32)))
        total += int((tri != NO_HIT).sum())
        # the scene path and the flattened dict are the same scene
        t2, d2 = oracle.closest_hits(c["scene_path"], o[:16], d[:16])
        assert np.array_equal(t2, tri[:16]) and np.array_equal(d2, dist[:16])
    assert total > 200


def test_all_rows_marked_equals_the_unrestricted_scan(run):
    c, ref, _ = run
    flat = oracle.flatten(oracle.read_hrt(c["scene_path"]))
    T = flat["tri_vtx"].shape[0]
    o, d = _states(c, ref, 1)
    full = oracle.closest_hits(flat, o, d)
    rng = np.random.default_rng(2)
    for order in (np.arange(T), rng.permutation(T)):   # rows of another table: any permutation of the flat indices
        W = (T + 63) // 64
        m = np.zeros((o.shape[0], W), np.uint64)
        for r in range(T):
            m[:, r >> 6] |= np.uint64(1) << np.uint64(r & 63)
        got = oracle.closest_hits(flat, o, d, m, order.astype(np.uint32))
        assert np.array_equal(got[0], full[0]) and np.array_equal(got[1], full[1])
    # nothing marked: nothing hit
    got = oracle.closest_hits(flat, o, d, np.zeros((o.shape[0], W), np.uint64), np.arange(T, dtype=np.uint32))
    assert (got[0] == NO_HIT).all()
    # a row past the table is an error, not a silent miss
    m = np.zeros((o.shape[0], W + 1), np.uint64)
    m[0, W] = 1 << 63
    with pytest.raises(RuntimeError):
        oracle.closest_hits(flat, o, d, m, np.arange(T, dtype=np.uint32))


def test_restricted_scan_visits_only_the_marked_rows(run):
    c, ref, _ = run
    flat = oracle.flatten(oracle.read_hrt(c["scene_path"]))
    T = flat["tri_vtx"].shape[0]
    o, d = _states(c, ref, 0)
    full = oracle.closest_hits(flat, o, d)
    order = np.random.default_rng(3).permutation(T).astype(np.uint32)
    inv = np.zeros(T, np.int64)
    inv[order] = np.arange(T)
    hit = np.flatnonzero(full[0] != NO_HIT)
    W = (T + 63) // 64
    m = np.full((o.shape[0], W), np.uint64(0xFFFFFFFFFFFFFFFF))
    for i in hit:   # everything but the winner's row
        r = int(inv[full[0][i]])
        m[i, r >> 6] &= ~(np.uint64(1) << np.uint64(r & 63))
    m[:, W - 1] &= np.uint64((1 << (T - 64 * (W - 1))) - 1) if T % 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    got = oracle.closest_hits(flat, o, d, m, order)
    assert (got[0][hit] != full[0][hit]).all()
    far = got[1][hit].view(np.float32) >= full[1][hit].view(np.float32)
    assert far.all()   # the runner-up is no closer


def test_tie_rule_lowest_flat_index(tmp_path):
    p = str(tmp_path / "nasty.hrt")
    G.nasty(p)   # the floor quad twice: flat indices 0, 1 and 2, 3 tie exactly
    flat = oracle.flatten(oracle.read_hrt(p))
    T = flat["tri_vtx"].shape[0]
    o = np.array([[3.0, -2.0, 4.0], [-7.0, 5.0, 2.0]], np.float32)
    d = np.array([[0.0, 0.0, -1.0], [0.1, 0.0, -1.0]], np.float32)
    full = oracle.closest_hits(flat, o, d)
    assert set(full[0]) <= {0, 1}
    order = np.arange(T, dtype=np.uint32)[::-1].copy()   # row r = flat index T - 1 - r
    m = np.zeros((2, 1), np.uint64)
    for f in (2, 3):   # only the duplicate quad
        m[:, 0] |= np.uint64(1) << np.uint64(T - 1 - f)
    dup = oracle.closest_hits(flat, o, d, m, order)
    assert np.array_equal(dup[0], full[0] + 2) and np.array_equal(dup[1], full[1])
    m[:, 0] |= np.uint64(0b11) << np.uint64(T - 2)   # and the original: the lower flat index wins again
    both = oracle.closest_hits(flat, o, d, m, order)
    assert np.array_equal(both[0], full[0]) and np.array_equal(both[1], full[1])


def test_shadow_dirs_are_the_runs_directions(run):
    c, ref, _ = run
    rx = np.asarray(c["rx_pos"], np.float32)
    n = c["num_paths"]
    seen = 0
    for b in range(c["num_bounces"]):
        o, _ = _states(c, ref, b + 1)   # the state after bounce b: the origin the shadow rays leave
        hit = ref["extras"]["hit_tri"][b, 0] != NO_HIT
        for k in range(rx.shape[0]):
            w = oracle.shadow_dirs(o, np.tile(rx[k], (n, 1)))
            got = ref["scat"]["directions_rx"][k, 0, b]
            a = ref["scat"]["a_te_re"][k, 0, b].view(np.uint32)
            unblocked = hit & (a != oracle.SENTINEL_U32) & ((a << 1) != 0)   # (a blocked record's direction is not written)
            assert np.array_equal((-w[unblocked]).view(np.uint32), got[unblocked].view(np.uint32))
            seen += int(unblocked.sum())
    assert seen > 100


def test_mirror_is_the_bounce(run):
    c, ref, _ = run
    flat = oracle.flatten(oracle.read_hrt(c["scene_path"]))
    o0, d0 = _states(c, ref, 0)
    o1, d1 = _states(c, ref, 1)
    tri = ref["extras"]["hit_tri"][0, 0]
    hit = np.flatnonzero(tri != NO_HIT)
    foot = (o1[hit].astype(np.float64) - 1e-4 * d1[hit]).astype(np.float32)   # where the ray met the triangle
    d, o = oracle.mirror(flat, tri[hit], o0[hit], foot, foot)
    assert np.abs(d.astype(np.float64) - d1[hit]).max() < 1e-5   # (d0 is re-formed from two points here: not the run's bits)
    assert np.abs(o.astype(np.float64) - o1[hit]).max() < 1e-4
    assert np.array_equal(o, foot + d * np.float32(1e-4))
    with pytest.raises(RuntimeError):
        oracle.mirror(flat, [flat["tri_vtx"].shape[0]], o0[:1], foot[:1], foot[:1])
