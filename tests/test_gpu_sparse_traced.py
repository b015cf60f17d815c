"""The array channel of traced dominant-path lists (Tracer.sparse_array_channel, Tracer.sparse_channel,
hrt_compute_sparse_array_channel, hermespy_rt.compute_sparse_array_channel) on box and simple_reflector with so few rays
that the list of K = 1 024 is COMPLETE on every link (kept = eligible, asserted from the header): the result is then
array_channel's.  Bounds, with S the link's sum of |a_p^pol| over the kept slots: 1e-5 S against the float64 reference of
the list (hermespy_rt_amd.sparse.reference), 2e-5 S against array_channel on the same grid -- the bound
tests/test_gpu_array_channel.py holds the same arithmetic to (each side within 1e-5 S of the float64 sum).  Then the
truncated list (K = 8), and the equivalences: the single-element form, merged shards, the drop-in entries in a child
process (once with forced batches), and svd() / equalizer() on the result.

The ray counts: a ray adds at most one record per bounce and link, so box (500 rays, 2 bounces) has at most 1 001
eligible terms per link and simple_reflector (2 500 rays, 3 bounces; the CPU oracle writes 613 records per link,
live rays 2 500 / 613 / 0 / 0) at most 614."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import dominant, sparse
from hermespy_rt_amd.workloads import cfg

from . import configs as K
from .dominant_util import to_numpy
from .pathsum_util import DF, _bits, _grid, _lam, _tracer, _ula, _upa

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NK, NT, DT = 24, 2, 1e-3
KMAX = 1024
CONFIGS = {
    "box": cfg("box.hrt", [[2, 1, 1.5], [5, 0, 2.5]], [[0, 0, 2.5], [1, 4, 1.0]], 3.0, 500, 2,
               rx_vel=[[1, 2, 3], [0, 0, 0]], tx_vel=[[10, 0, 0], [0, -5, 0]]),
    "simple_reflector": cfg("simple_reflector.hrt", [[-.3, .2, .4], [2, 0, .5]], [[.2, .1, .3]], 3.0, 2500, 3,
                            rx_vel=[[0, 0, 0], [3, 0, 1]], tx_vel=[[0, 2, 0]]),
}


def _geometry(c):
    lam = _lam(c)
    return _upa(3, 4, lam / 2), _ula(5, lam / 2, axis=0)       # 60 pairs: two pair blocks, the second partial


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def traced(request):
    c = CONFIGS[request.param]
    tr = _tracer(c)
    tr.trace()
    tr.torch.cuda.synchronize(tr.device)
    yield tr, c
    tr.close()


def _s(S):
    return S[:, :, None, None, :, None, None]


def _ft(c):
    f0 = _grid(c, NK)
    return f0, f0 + DF * np.arange(NK), DT * np.arange(NT)


def test_complete_lists_give_the_array_channel(traced):
    tr, c = traced
    dp = tr.dominant_paths(KMAX)
    v = to_numpy(dp)
    kept, el = v["kept"].astype(np.int64), v["eligible"].astype(np.int64)
    print("eligible per link", el.tolist())
    assert np.array_equal(kept, el) and (el <= KMAX).all(), (kept.tolist(), el.tolist())   # every link, none skipped
    assert (el > 32).all()                                                                 # more than one batch each
    rxe, txe = _geometry(c)
    f0, f, t = _ft(c)
    fa = c["f_ghz"] * 1e9
    H = tr.sparse_array_channel(dp, rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
    assert tuple(H.shape) == (tr.nrx, tr.ntx, 12, 5, 2, NT, NK)
    ref, S = sparse.reference(v, rxe, txe, fa, f, t)
    assert (S > 0).all()
    got = H.cpu().numpy()
    e1 = np.abs(got - ref) / _s(S)
    A = tr.array_channel(rxe, txe, f0, DF, NK, dt=DT, num_times=NT).cpu().numpy()
    e2 = np.abs(got - A) / _s(S)
    print("worst |H - ref| / S = %.3g, worst |H - array_channel| / S = %.3g" % (e1.max(), e2.max()))
    assert (e1 <= 1e-5).all(), e1.max()
    assert (e2 <= 2e-5).all(), e2.max()
    assert np.abs(ref).max() > 1e-3 * S.max()


def test_truncated_lists_give_the_channel_of_the_kept_slots(traced):
    tr, c = traced
    dp = tr.dominant_paths(8)
    v = to_numpy(dp)
    assert (v["kept"] == 8).all() and (v["eligible"].astype(np.int64) > 8).all()
    rxe, txe = _geometry(c)
    f0, f, t = _ft(c)
    H = tr.sparse_array_channel(dp, rxe, txe, f0, DF, NK, dt=DT, num_times=NT).cpu().numpy()
    ref, S = sparse.reference(v, rxe, txe, c["f_ghz"] * 1e9, f, t)
    live = np.arange(8) < v["kept"].astype(np.int64)[..., None]
    assert np.allclose(S[..., 0], np.where(live, np.abs(v["a_te"]), 0).sum(-1))
    e = np.abs(H - ref) / _s(S)
    print("K = 8: worst |H - ref| / S_kept = %.3g" % e.max())
    assert (e <= 1e-5).all(), e.max()
    # the power the list leaves out is what power_profiles has beyond the kept slots
    m = tr.power_profiles(0.0, 1e-9, 1)["moments"].cpu().numpy()
    d = sparse.dropped_power(v, m)
    frac = dominant.captured_fraction(v, m)
    assert (d > 0).all() and np.allclose(1.0 - frac, d / (d + np.where(live, v["power"], 0).sum(-1)))


def test_single_element_form_is_the_array_form_at_one_zero_offset_element(traced):
    tr, c = traced
    dp = tr.dominant_paths(64)
    f0, _, _ = _ft(c)
    z = np.zeros((1, 3))
    a = tr.sparse_channel(dp, f0, DF, NK, dt=DT, num_times=NT)
    b = tr.sparse_array_channel(dp, z, z, f0, DF, NK, dt=DT, num_times=NT)
    assert tuple(a.shape) == (tr.nrx, tr.ntx, 2, NT, NK)
    assert tr.torch.equal(_bits(a), _bits(b[:, :, 0, 0])) and float(a.abs().max()) > 0
    # and it is channel() of the kept terms: with a complete list, channel() itself within the two bounds
    dpc = tr.dominant_paths(KMAX)
    v = to_numpy(dpc)
    S = np.stack([np.abs(v["a_te"]).sum(-1), np.abs(v["a_tm"]).sum(-1)], -1)[:, :, :, None, None]
    s = tr.sparse_channel(dpc, f0, DF, NK, dt=DT, num_times=NT).cpu().numpy()
    h = tr.channel(f0, DF, NK, dt=DT, num_times=NT).cpu().numpy()
    assert (np.abs(s - h) <= 2e-5 * S).all()


def test_merged_shards_give_the_unsharded_bytes(traced):
    tr, c = traced
    rxe, txe = _geometry(c)
    f0, _, _ = _ft(c)
    for k in (8, KMAX):
        whole = tr.sparse_array_channel(tr.dominant_paths(k), rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
        sep = []
        for r in range(2):
            ts = _tracer(c, rank=r, world=2, chunk=64)
            ts.trace()
            sep.append(to_numpy(ts.dominant_paths(k)))
            ts.close()
        merged = dominant.merge(sep[1], sep[0])            # a numpy result: uploaded
        assert isinstance(merged["buffer"], np.ndarray)
        got = tr.sparse_array_channel(merged, rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
        assert tr.torch.equal(_bits(got), _bits(whole)), k


_DROP_IN_CALL = """
import sys
import numpy as np
sys.path.insert(0, {repo!r})
import torch  # noqa: F401
import hermespy_rt_amd
sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
import hermespy_rt
from hermespy_rt_amd import abi, lib
from tests import configs as K
c = K.small(K.C3, 20000)
rxe, txe = np.load(sys.argv[2]).astype(np.float32), np.load(sys.argv[3]).astype(np.float32)
args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
        np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], len(c["rx_pos"]),
        len(c["tx_pos"]), c["num_paths"], c["num_bounces"], {f0!r}, {df!r}, {nk}, rxe, txe, {k})
kw = dict(dt={dt!r}, num_times={nt})
H = hermespy_rt.compute_sparse_array_channel(*args, **kw)
H2, d = hermespy_rt.compute_sparse_array_channel(*args, return_paths=True, **kw)
assert H.dtype == np.complex64 and np.array_equal(H.view(np.uint8), H2.view(np.uint8))
st = lib.Stats()
H3, d3 = abi.run_compute_sparse_array_channel(lib.load(), *K.args(c), abi.dominant_spec({k}),
                                              abi.channel_spec({f0!r}, {df!r}, {nk}, 0.0, {dt!r}, {nt}), rxe, txe,
                                              return_paths=True, stats=st)
assert np.array_equal(H.view(np.uint8), H3.view(np.uint8)) and np.array_equal(d["buffer"], d3["buffer"])
d4 = hermespy_rt.compute_dominant_paths(*args[:10], {k})
assert np.array_equal(d["buffer"], d4["buffer"])
np.save(sys.argv[1], H)
np.save(sys.argv[4], d["buffer"])
print("batches", int(st.num_batches))
"""


@pytest.mark.parametrize("batched", [False, True], ids=["one_batch", "batched"])
def test_drop_in_entries_equal_the_tracer_route(tmp_path, batched):
    """the drop-in entries (pybind and C, bitwise equal; a fresh child process runs them) return the bytes
    sparse_array_channel(dominant_paths(K)) gives, and the lists compute_dominant_paths gives"""
    k = 64
    c = K.small(K.C3, 20000)      # (large enough for the batch loop to split)
    f0, _, _ = _ft(c)
    rxe, txe = _geometry(c)
    tr = _tracer(c)
    tr.trace()
    dp = tr.dominant_paths(k)
    want = tr.sparse_array_channel(dp, rxe, txe, f0, DF, NK, dt=DT, num_times=NT).cpu().numpy()
    lists = to_numpy(dp)
    live = lists["bounce"] >= 0
    lists["tri"][live] = tr.tri_order[lists["tri"][live]]     # the host entries report the reference's flat index
    env = dict(os.environ)
    if batched:   # a budget below one workspace of the whole launch set
        env["HRT_WORKSPACE_BYTES"] = str(int(tr.ws.numel()) * 2 // 3)
    tr.close()
    files = [tmp_path / n for n in ("h.npy", "rx.npy", "tx.npy", "lists.npy")]
    np.save(files[1], rxe)
    np.save(files[2], txe)
    p = subprocess.run([sys.executable, "-c", _DROP_IN_CALL.format(repo=REPO, f0=f0, df=DF, nk=NK, dt=DT,
                                                                   nt=NT, k=k)] + [str(x) for x in files],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    batches = int(p.stdout.split()[-1])
    assert batches >= 2 if batched else batches == 1
    H = np.load(files[0])
    assert H.shape == want.shape and np.array_equal(H.view(np.uint8), want.view(np.uint8)) and np.abs(H).max() > 0
    assert np.array_equal(np.load(files[3]), lists["buffer"])


def test_svd_and_equalizer_accept_the_result(traced):
    tr, c = traced
    lam = _lam(c)
    rxe, txe = _upa(2, 4, lam / 2), _ula(4, lam / 2, axis=0)
    f0, _, _ = _ft(c)
    H = tr.sparse_array_channel(tr.dominant_paths(64), rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
    s = tr.svd(H)
    assert tuple(s["sigma"].shape) == (tr.nrx, tr.ntx, 4, 2, NT, NK) and float(s["sigma"][:, :, 0].min()) > 0
    fro = (H.abs() ** 2).sum(dim=(2, 3))
    assert tr.torch.allclose((s["sigma"] ** 2).sum(dim=2), fro, rtol=1e-4)
    e = tr.equalizer(H, noise=1e-12, kind="lmmse")
    assert bool(tr.torch.isfinite(e["sinr"]).all()) and float(e["sinr"].max()) > 0
