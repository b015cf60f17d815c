"""oracle.scatter_records -- the oracle's per-receiver scatter loop as a callable (oracle/hrt_oracle.c
scatter_to_receivers; the reference of tests/test_gpu_records_planted.py) -- against the whole-path oracle that calls the
same function and is pinned to the reference by tests/test_oracle_*.py: fed with the states of bounce 0 that
compute_paths reports (the snapshot's o and d, hit_tri, hit_theta, hit_state), it must reproduce the dense scatter arrays
of that bounce bit for bit, written and unwritten slots alike.  No GPU."""
import numpy as np
import pytest

from oracle import oracle

from . import configs as K

CASES = dict(
    box=dict(K.small(K.IN_PLANE["box"], 2001), num_bounces=2, tx_vel=[[10.0, -3.0, 2.0]]),
    simple_reflector=dict(K.small(K.TEST_PY, 3001), rx_pos=[[0, 0, .15], [.3, .2, .5], [-2, 1, .01]], rx_vel=[K.Z] * 3,
                          tx_vel=[[0.0, 5.0, 1.0]]),
)
FIELDS = ("a_te_re", "a_te_im", "a_tm_re", "a_tm_im", "tau")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(CASES))
def test_scatter_records_reproduce_bounce0(name):
    c = CASES[name]
    ref = oracle.compute_paths(*K.args(c))
    ex, npth, nb = ref["extras"], c["num_paths"], c["num_bounces"]
    nrx = len(c["rx_pos"])
    assert len(c["tx_pos"]) == 1
    hit = np.flatnonzero(ex["hit_tri"][0, 0] != oracle.NO_HIT)
    assert hit.size > 100
    # the state after bounce 0: snapshot 1 of the rays (o already advanced, d mirrored), and what the extras carry
    snap = ref["scat_rays"][npth:2 * npth][hit]
    st = ex["hit_state"][0, 0][hit]
    states = dict(o=snap[:, :3], d=snap[:, 3:], tri=ex["hit_tri"][0, 0][hit], theta=ex["hit_theta"][0, 0][hit],
                  amp=st[:, :4], tau=st[:, 4])
    got = oracle.scatter_records(c["scene_path"], c["f_ghz"], c["rx_pos"], states)
    ub = got["unblocked"]
    assert ub.any() and nrx == 3
    dense = ref["scat"]
    for k in FIELDS:   # blocked records: five zeros; unblocked: the values -- and nothing written anywhere else
        want = dense[k][:, 0, 0, :]
        assert np.array_equal(_bits(want[:, hit]), _bits(got[k])), k
        rest = np.delete(_bits(want), hit, axis=1)
        assert (rest == oracle.SENTINEL_U32).all(), k
    d = dense["directions_rx"][:, 0, 0, :, :][:, hit]
    for j, k in enumerate(("dirx", "diry", "dirz")):   # (a blocked record's direction: the sentinel on both sides)
        assert np.array_equal(_bits(d[..., j]), _bits(got[k])), k
    # freq_shift = launch term - the record's (unblocked records; one TX, so the dense fill is the launch term, and the
    # Q10 term added to the slots of RX 0 is dot(d - d, mvel) = 0)
    dirs = ex["launch_dirs"][hit]
    tv = np.asarray(c["tx_vel"], np.float32)[0]
    f_hz = np.float32(np.float64(np.float32(c["f_ghz"])) * 1e9)
    dop = f_hz / np.float32(299792458.0)
    fs0 = ((tv[0] * dirs[:, 0] + tv[1] * dirs[:, 1]) + tv[2] * dirs[:, 2]) * dop
    assert fs0.dtype == np.float32 and np.any(fs0 != 0)
    fs = dense["freq_shift"][:, 0, 0, :][:, hit]
    assert np.array_equal(fs[ub], (fs0[None, :] - got["dfs"])[ub])
    assert np.array_equal(fs[~ub], np.broadcast_to(fs0, fs.shape)[~ub])
    assert (_bits(got["dfs"])[~ub] == oracle.SENTINEL_U32).all()


def test_scatter_records_refuses_rows_past_the_table():
    c = CASES["box"]
    st = dict(o=[[0, 0, 1]], d=[[0, 0, 1]], tri=[10 ** 6], theta=[0.1], amp=[[1, 0, 1, 0]], tau=[0.0])
    with pytest.raises(RuntimeError):
        oracle.scatter_records(c["scene_path"], c["f_ghz"], c["rx_pos"], st)
