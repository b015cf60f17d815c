"""The array taps of traced dominant-path lists (Tracer.sparse_array_taps, Tracer.sparse_taps,
hrt_compute_sparse_array_taps, hermespy_rt.compute_sparse_array_taps) on box and simple_reflector with so few rays that
the list of K = 1 024 is COMPLETE on every link (kept = eligible, asserted from the header): the result is then
array_taps'.  Bounds, with S the link's sum of |a_p^pol| over the kept slots: 1e-5 S against the float64 reference of
the list (hermespy_rt_amd.sparse.taps_reference), 2e-5 S against array_taps on the same trace -- the bound
tests/test_gpu_array_taps.py holds the same arithmetic to (each side within 1e-5 S of the float64 sum).  Then the
truncated list (K = 8), and the equivalences: the single-element form, merged shards, the drop-in entries in a child
process (once with forced batches), apply_taps on the result and beams.apply of it.  The scenes and ray counts are
tests/test_gpu_sparse_traced.py's."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import beams, dominant, sparse
from hermespy_rt_amd import propagate as pg

from . import configs as K
from .dominant_util import to_numpy
from .pathsum_util import FS, _bits, _lam, _tracer, _ula, _upa
from .test_gpu_sparse_traced import CONFIGS, KMAX

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_TAPS, L_MIN, NT, DT = 40, -6, 2, 1e-3


def _geometry(c):
    lam = _lam(c)
    return _upa(3, 4, lam / 2), _ula(5, lam / 2, axis=0)       # 60 pairs x 2 times: two row blocks, the second partial


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


def _kw(c):
    return dict(fs=FS, num_taps=L_TAPS, l_min=L_MIN, fc=c["f_ghz"] * 1e9, dt=DT, num_times=NT)


def _lt():
    return L_MIN + np.arange(L_TAPS), DT * np.arange(NT)


def test_complete_lists_give_the_array_taps(traced):
    tr, c = traced
    dp = tr.dominant_paths(KMAX)
    v = to_numpy(dp)
    kept, el = v["kept"].astype(np.int64), v["eligible"].astype(np.int64)
    print("eligible per link", el.tolist())
    assert np.array_equal(kept, el) and (el <= KMAX).all(), (kept.tolist(), el.tolist())   # every link, none skipped
    assert (el > 32).all()                                                                 # more than one batch each
    rxe, txe = _geometry(c)
    l, t = _lt()
    fa = fc = c["f_ghz"] * 1e9
    h = tr.sparse_array_taps(dp, rxe, txe, **_kw(c))
    assert tuple(h.shape) == (tr.nrx, tr.ntx, 12, 5, 2, NT, L_TAPS)
    ref, S = sparse.taps_reference(v, rxe, txe, fa, FS, fc, l, t)
    assert (S > 0).all()
    got = h.cpu().numpy()
    e1 = np.abs(got - ref) / _s(S)
    A = tr.array_taps(rxe, txe, FS, L_TAPS, L_MIN, dt=DT, num_times=NT).cpu().numpy()
    e2 = np.abs(got - A) / _s(S)
    print("worst |h - ref| / S = %.3g, worst |h - array_taps| / S = %.3g" % (e1.max(), e2.max()))
    assert (e1 <= 1e-5).all(), e1.max()
    assert (e2 <= 2e-5).all(), e2.max()
    assert np.abs(ref).max() > 1e-3 * S.max()


def test_truncated_lists_give_the_taps_of_the_kept_slots(traced):
    tr, c = traced
    dp = tr.dominant_paths(8)
    v = to_numpy(dp)
    assert (v["kept"] == 8).all() and (v["eligible"].astype(np.int64) > 8).all()
    rxe, txe = _geometry(c)
    l, t = _lt()
    h = tr.sparse_array_taps(dp, rxe, txe, **_kw(c)).cpu().numpy()
    ref, S = sparse.taps_reference(v, rxe, txe, c["f_ghz"] * 1e9, FS, c["f_ghz"] * 1e9, l, t)
    live = np.arange(8) < v["kept"].astype(np.int64)[..., None]
    assert np.allclose(S[..., 0], np.where(live, np.abs(v["a_te"]), 0).sum(-1))
    e = np.abs(h - ref) / _s(S)
    print("K = 8: worst |h - ref| / S_kept = %.3g" % e.max())
    assert (e <= 1e-5).all(), e.max()
    assert np.abs(ref).max() > 1e-3 * S.max()


def test_single_element_form_is_the_array_form_at_one_zero_offset_element(traced):
    tr, c = traced
    dp = tr.dominant_paths(64)
    z = np.zeros((1, 3))
    a = tr.sparse_taps(dp, **_kw(c))
    b = tr.sparse_array_taps(dp, z, z, **_kw(c))
    assert tuple(a.shape) == (tr.nrx, tr.ntx, 2, NT, L_TAPS)
    assert tr.torch.equal(_bits(a), _bits(b[:, :, 0, 0])) and float(a.abs().max()) > 0
    # and it is taps() of the kept terms: with a complete list, taps() itself within the two bounds
    dpc = tr.dominant_paths(KMAX)
    v = to_numpy(dpc)
    S = np.stack([np.abs(v["a_te"]).sum(-1), np.abs(v["a_tm"]).sum(-1)], -1)[:, :, :, None, None]
    s = tr.sparse_taps(dpc, **_kw(c)).cpu().numpy()
    h = tr.taps(FS, L_TAPS, L_MIN, dt=DT, num_times=NT).cpu().numpy()
    assert (np.abs(s - h) <= 2e-5 * S).all()


def test_merged_shards_give_the_unsharded_bytes(traced):
    tr, c = traced
    rxe, txe = _geometry(c)
    for k in (8, KMAX):
        whole = tr.sparse_array_taps(tr.dominant_paths(k), rxe, txe, **_kw(c))
        sep = []
        for r in range(2):
            ts = _tracer(c, rank=r, world=2, chunk=64)
            ts.trace()
            sep.append(to_numpy(ts.dominant_paths(k)))
            ts.close()
        merged = dominant.merge(sep[1], sep[0])            # a numpy result: uploaded
        assert isinstance(merged["buffer"], np.ndarray)
        got = tr.sparse_array_taps(merged, rxe, txe, **_kw(c))
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
        len(c["tx_pos"]), c["num_paths"], c["num_bounces"], {fs!r}, {nl}, rxe, txe, {k})
kw = dict(l_min={l_min}, dt={dt!r}, num_times={nt})
h = hermespy_rt.compute_sparse_array_taps(*args, **kw)
h2, d = hermespy_rt.compute_sparse_array_taps(*args, return_paths=True, **kw)
assert h.dtype == np.complex64 and np.array_equal(h.view(np.uint8), h2.view(np.uint8))
st = lib.Stats()
h3, d3 = abi.run_compute_sparse_array_taps(lib.load(), *K.args(c), abi.dominant_spec({k}),
                                           abi.taps_spec({fs!r}, {nl}, {l_min}, c["f_ghz"] * 1e9, 0.0, {dt!r}, {nt}),
                                           rxe, txe, return_paths=True, stats=st)
assert np.array_equal(h.view(np.uint8), h3.view(np.uint8)) and np.array_equal(d["buffer"], d3["buffer"])
d4 = hermespy_rt.compute_dominant_paths(*args[:10], {k})
assert np.array_equal(d["buffer"], d4["buffer"])
np.save(sys.argv[1], h)
np.save(sys.argv[4], d["buffer"])
print("batches", int(st.num_batches))
"""


@pytest.mark.parametrize("batched", [False, True], ids=["one_batch", "batched"])
def test_drop_in_entries_equal_the_tracer_route(tmp_path, batched):
    """the drop-in entries (pybind and C, bitwise equal; a fresh child process runs them) return the bytes
    sparse_array_taps(dominant_paths(K)) gives, and the lists compute_dominant_paths gives"""
    k = 64
    c = K.small(K.C3, 20000)      # (large enough for the batch loop to split)
    rxe, txe = _geometry(c)
    tr = _tracer(c)
    tr.trace()
    dp = tr.dominant_paths(k)
    want = tr.sparse_array_taps(dp, rxe, txe, **_kw(c)).cpu().numpy()
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
    p = subprocess.run([sys.executable, "-c", _DROP_IN_CALL.format(repo=REPO, fs=FS, nl=L_TAPS, l_min=L_MIN, dt=DT,
                                                                   nt=NT, k=k)] + [str(x) for x in files],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    batches = int(p.stdout.split()[-1])
    assert batches >= 2 if batched else batches == 1
    h = np.load(files[0])
    assert h.shape == want.shape and np.array_equal(h.view(np.uint8), want.view(np.uint8)) and np.abs(h).max() > 0
    assert np.array_equal(np.load(files[3]), lists["buffer"])


def test_apply_taps_and_beams_accept_the_result(traced):
    """the result goes into apply_taps as it is: the bytes of a copy of the same tensor made through the host, and the
    float64 per-path received signal within the tolerance of tests/test_gpu_propagate_traced.py (1e-5 S per tap carried
    through sum |x| over the tap window of every TX port, plus propagate.error_bound); beams.apply contracts it"""
    tr, c = traced
    torch = tr.torch
    lam = _lam(c)
    rxe, txe = _ula(2, lam / 2), _ula(3, lam / 2, axis=0)
    dp = tr.dominant_paths(64)
    v = to_numpy(dp)
    fc = c["f_ghz"] * 1e9
    h = tr.sparse_array_taps(dp, rxe, txe, FS, L_TAPS, L_MIN, fc)
    n = 48
    rng = np.random.RandomState(4)
    x = (rng.standard_normal((tr.ntx, 3, n)) + 1j * rng.standard_normal((tr.ntx, 3, n))).astype(np.complex64)
    xd = torch.from_numpy(x).to(tr.device)
    y = tr.apply_taps(h, xd, L_MIN)
    n_out = pg.default_num_out(n, L_TAPS, L_MIN)
    assert tuple(y.shape) == (tr.nrx, 2, 2, n_out)
    y2 = tr.apply_taps(torch.from_numpy(h.cpu().numpy().copy()).to(tr.device), xd, L_MIN)
    assert torch.equal(_bits(y), _bits(y2))
    h64, S = sparse.taps_reference(v, rxe, txe, fc, FS, fc, L_MIN + np.arange(L_TAPS), [0.0])
    ref = pg.apply_taps_reference(h64, x, L_MIN, None, n_out)
    ones = np.ones(h64.shape) * (1e-5 * S)[:, :, None, None, :, None, None]
    tol = pg.apply_taps_reference(ones, np.abs(x), L_MIN, None, n_out).real + pg.error_bound(h64, x, L_MIN, None, n_out)
    got = y.cpu().numpy().astype(np.complex128)
    err = np.maximum(np.abs(got.real - ref.real), np.abs(got.imag - ref.imag))
    live = tol > 0
    assert live.any() and not ref[~live].any() and not got[~live].any() and np.abs(ref).max() > 0
    print("largest error / tolerance: %.3f" % (err[live] / tol[live]).max())
    assert (err[live] <= tol[live]).all()
    # beams.apply: the contraction of the float64 taps within 1e-5 S sum |w_rx| sum |w_tx|
    wr = np.exp(2j * np.pi * np.outer(np.arange(2), np.arange(2)) / 2).astype(np.complex64)
    wt = np.exp(2j * np.pi * np.outer(np.arange(2), np.arange(3)) / 3).astype(np.complex64)
    B = beams.apply(h.cpu().numpy().astype(np.complex128), wr, wt)
    assert B.shape == (tr.nrx, tr.ntx, 2, 2, 2, 1, L_TAPS)
    e = np.abs(h.cpu().numpy() - h64) / _s(S)
    print("K = 64: worst |h - ref| / S_kept = %.3g" % e.max())
    assert (e <= 1e-5).all()
    assert (np.abs(B - beams.apply(h64, wr, wt)) <= (1 + 1e-9) * 1e-5 * 2 * 3 * _s(S)).all() and np.abs(B).max() > 0
