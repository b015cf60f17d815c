"""The beam taps of traced dominant-path lists (Tracer.sparse_beam_taps, hrt_compute_sparse_beam_taps,
hermespy_rt.compute_sparse_beam_taps) on the scenes and sizes of tests/test_gpu_sparse_traced.py: box and
simple_reflector with so few rays that the list of K = 1 024 is COMPLETE on every link (kept = eligible, asserted from
the header), so the result is then beam_taps'.  Bounds, with S the link's sum of |a_p^pol| over the kept slots and
N = ||W_rx[a]||_1 ||W_tx[b]||_1: 1e-5 N S against the float64 reference of the list
(hermespy_rt_amd.sparse.beam_taps_reference; tests/beam_util.py bound, the project's own tolerance), 2e-5 N S against
Tracer.beam_taps on the same trace and against beams.apply of sparse_array_taps (two device results, each within
1e-5 N S of the float64 sum).  With identity codebooks N = 1 and h[a, b] is sparse_array_taps' h[i, j]: 2e-5 S.  Then
the truncated list (K = 8), the shape the array taps of a list refuse, merged shards, the drop-in entries in a child
process (once with forced batches), and apply_taps on the result.

Measured on an MI355X (largest error over bound): see DESIGN section 26."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import beams, dominant, sparse
from hermespy_rt_amd import propagate as pg

from . import beam_util as BU
from . import configs as K
from .dominant_util import to_numpy
from .pathsum_util import FS, _bits, _lam, _tracer, _ula, _upa
from .test_gpu_sparse_traced import CONFIGS, KMAX

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_TAPS, L_MIN, NT, DT = 40, -6, 2, 1e-3


def _geometry(c):
    lam = _lam(c)
    return _upa(3, 4, lam / 2), _ula(5, lam / 2, axis=0)


def _codebooks():
    return BU.random_weights(7, 12, 61), BU.random_weights(6, 5, 62)     # 42 pairs x 2 times: two row blocks


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def traced(request):
    c = CONFIGS[request.param]
    tr = _tracer(c)
    tr.trace()
    tr.torch.cuda.synchronize(tr.device)
    yield tr, c
    tr.close()


def _kw(c, L=L_TAPS, nt=NT):
    return dict(fs=FS, num_taps=L, l_min=L_MIN, fc=c["f_ghz"] * 1e9, dt=DT, num_times=nt)


def _lt(L=L_TAPS, nt=NT):
    return L_MIN + np.arange(L), DT * np.arange(nt)


def test_complete_lists_give_the_beam_taps(traced):
    tr, c = traced
    dp = tr.dominant_paths(KMAX)
    v = to_numpy(dp)
    kept, el = v["kept"].astype(np.int64), v["eligible"].astype(np.int64)
    assert np.array_equal(kept, el) and (el <= KMAX).all(), (kept.tolist(), el.tolist())   # every link, none skipped
    assert (el > 32).all()                                                                 # more than one batch each
    rxe, txe = _geometry(c)
    wr, wt = _codebooks()
    l, t = _lt()
    fa = fc = c["f_ghz"] * 1e9
    h = tr.sparse_beam_taps(dp, rxe, txe, wr, wt, **_kw(c))
    assert tuple(h.shape) == (tr.nrx, tr.ntx, 7, 6, 2, NT, L_TAPS)
    ref, S = sparse.beam_taps_reference(v, rxe, txe, wr, wt, fa, FS, fc, l, t)
    assert (S > 0).all() and np.abs(ref).max() > 1e-3 * S.max()
    got = h.cpu().numpy()
    BU.check(got, ref, S, wr, wt, 1e-5, "sparse_beam_taps vs float64")
    full = tr.beam_taps(rxe, txe, wr, wt, FS, L_TAPS, L_MIN, dt=DT, num_times=NT).cpu().numpy()
    BU.check(got, full.astype(np.complex128), S, wr, wt, 2e-5, "sparse_beam_taps vs beam_taps")
    he = tr.sparse_array_taps(dp, rxe, txe, **_kw(c)).cpu().numpy().astype(np.complex128)
    BU.check(got, beams.apply(he, wr, wt), S, wr, wt, 2e-5, "sparse_beam_taps vs beams.apply(sparse_array_taps)")


def test_truncated_lists_give_the_beam_taps_of_the_kept_slots(traced):
    tr, c = traced
    dp = tr.dominant_paths(8)
    v = to_numpy(dp)
    assert (v["kept"] == 8).all() and (v["eligible"].astype(np.int64) > 8).all()
    rxe, txe = _geometry(c)
    wr, wt = _codebooks()
    l, t = _lt()
    h = tr.sparse_beam_taps(dp, rxe, txe, wr, wt, **_kw(c)).cpu().numpy()
    ref, S = sparse.beam_taps_reference(v, rxe, txe, wr, wt, c["f_ghz"] * 1e9, FS, c["f_ghz"] * 1e9, l, t)
    assert np.allclose(S[..., 0], np.abs(v["a_te"]).sum(-1))
    BU.check(h, ref, S, wr, wt, 1e-5, "K = 8 vs float64 over the kept slots")


def test_identity_codebooks_give_the_array_taps_of_the_list(traced):
    tr, c = traced
    dp = tr.dominant_paths(KMAX)
    v = to_numpy(dp)
    rxe, txe = _geometry(c)
    wr, wt = np.eye(12, dtype=np.complex64), np.eye(5, dtype=np.complex64)
    l, t = _lt()
    h = tr.sparse_beam_taps(dp, rxe, txe, wr, wt, **_kw(c)).cpu().numpy()
    he = tr.sparse_array_taps(dp, rxe, txe, **_kw(c)).cpu().numpy()
    _, S = sparse.taps_reference(v, rxe, txe, c["f_ghz"] * 1e9, FS, c["f_ghz"] * 1e9, l[:1], t[:1])
    BU.check(h, he.astype(np.complex128), S, wr, wt, 2e-5, "identity codebooks vs sparse_array_taps")
    assert np.abs(he).max() > 1e-3 * S.max()


def test_256_by_256_elements_are_accepted_where_the_array_taps_of_the_list_are_refused(traced):
    tr, c = traced
    lam = _lam(c)
    dp = tr.dominant_paths(KMAX)
    v = to_numpy(dp)
    rxe, txe = _upa(16, 16, lam / 2), _upa(16, 16, lam / 2)[:, [2, 1, 0]]
    wr, wt = BU.random_weights(4, 256, 71), BU.random_weights(4, 256, 72)
    nl = 512
    l, t = _lt(nl, 1)
    with pytest.raises(ValueError, match=r"hrt_sparse_array_taps: .*2\^24"):
        tr.sparse_array_taps(dp, rxe, txe, **_kw(c, nl, 1))
    h = tr.sparse_beam_taps(dp, rxe, txe, wr, wt, **_kw(c, nl, 1))
    assert tuple(h.shape) == (tr.nrx, tr.ntx, 4, 4, 2, 1, nl)
    ref, S = sparse.beam_taps_reference(v, rxe, txe, wr, wt, c["f_ghz"] * 1e9, FS, c["f_ghz"] * 1e9, l, t)
    BU.check(h.cpu().numpy(), ref, S, wr, wt, 1e-5, "256 x 256 elements, 4 x 4 beams, L = 512")


def test_merged_shards_give_the_unsharded_bytes(traced):
    tr, c = traced
    rxe, txe = _geometry(c)
    wr, wt = _codebooks()
    for k in (8, KMAX):
        whole = tr.sparse_beam_taps(tr.dominant_paths(k), rxe, txe, wr, wt, **_kw(c))
        sep = []
        for r in range(2):
            ts = _tracer(c, rank=r, world=2, chunk=64)
            ts.trace()
            sep.append(to_numpy(ts.dominant_paths(k)))
            ts.close()
        merged = dominant.merge(sep[1], sep[0])            # a numpy result: uploaded
        assert isinstance(merged["buffer"], np.ndarray)
        got = tr.sparse_beam_taps(merged, rxe, txe, wr, wt, **_kw(c))
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
wr, wt = np.load(sys.argv[5]), np.load(sys.argv[6])
args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
        np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], len(c["rx_pos"]),
        len(c["tx_pos"]), c["num_paths"], c["num_bounces"], {fs!r}, {nl}, rxe, txe, wr, wt, {k})
kw = dict(l_min={l_min}, dt={dt!r}, num_times={nt})
h = hermespy_rt.compute_sparse_beam_taps(*args, **kw)
h2, d = hermespy_rt.compute_sparse_beam_taps(*args, return_paths=True, **kw)
assert h.dtype == np.complex64 and np.array_equal(h.view(np.uint8), h2.view(np.uint8))
st = lib.Stats()
h3, d3 = abi.run_compute_sparse_beam_taps(lib.load(), *K.args(c), abi.dominant_spec({k}),
                                          abi.taps_spec({fs!r}, {nl}, {l_min}, c["f_ghz"] * 1e9, 0.0, {dt!r}, {nt}),
                                          rxe, txe, wr, wt, return_paths=True, stats=st)
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
    sparse_beam_taps(dominant_paths(K)) gives, and the lists dominant_paths gives"""
    k = 64
    c = K.small(K.C3, 20000)      # (large enough for the batch loop to split)
    rxe, txe = _geometry(c)
    wr, wt = _codebooks()
    tr = _tracer(c)
    tr.trace()
    dp = tr.dominant_paths(k)
    want = tr.sparse_beam_taps(dp, rxe, txe, wr, wt, **_kw(c)).cpu().numpy()
    lists = to_numpy(dp)
    live = lists["bounce"] >= 0
    lists["tri"][live] = tr.tri_order[lists["tri"][live]]     # the host entries report the reference's flat index
    env = dict(os.environ)
    if batched:   # a budget below one workspace of the whole launch set
        env["HRT_WORKSPACE_BYTES"] = str(int(tr.ws.numel()) * 2 // 3)
    tr.close()
    files = [tmp_path / n for n in ("h.npy", "rx.npy", "tx.npy", "lists.npy", "wr.npy", "wt.npy")]
    for path, a in zip((files[1], files[2], files[4], files[5]), (rxe, txe, wr, wt)):
        np.save(path, a)
    p = subprocess.run([sys.executable, "-c", _DROP_IN_CALL.format(repo=REPO, fs=FS, nl=L_TAPS, l_min=L_MIN, dt=DT,
                                                                   nt=NT, k=k)] + [str(x) for x in files],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    batches = int(p.stdout.split()[-1])
    assert batches >= 2 if batched else batches == 1
    h = np.load(files[0])
    assert h.shape == want.shape and np.array_equal(h.view(np.uint8), want.view(np.uint8)) and np.abs(h).max() > 0
    assert np.array_equal(np.load(files[3]), lists["buffer"])


def test_apply_taps_accepts_the_result(traced):
    """the result goes into apply_taps as it is, one waveform per TX beam: the bytes of a copy of the same tensor made
    through the host"""
    tr, c = traced
    torch = tr.torch
    rxe, txe = _geometry(c)
    wr, wt = BU.random_weights(2, 12, 81), BU.random_weights(3, 5, 82)
    h = tr.sparse_beam_taps(tr.dominant_paths(64), rxe, txe, wr, wt, FS, L_TAPS, L_MIN, c["f_ghz"] * 1e9)
    n = 48
    rng = np.random.RandomState(4)
    x = (rng.standard_normal((tr.ntx, 3, n)) + 1j * rng.standard_normal((tr.ntx, 3, n))).astype(np.complex64)
    xd = torch.from_numpy(x).to(tr.device)
    y = tr.apply_taps(h, xd, L_MIN)
    assert tuple(y.shape) == (tr.nrx, 2, 2, pg.default_num_out(n, L_TAPS, L_MIN)) and float(y.abs().max()) > 0
    y2 = tr.apply_taps(torch.from_numpy(h.cpu().numpy().copy()).to(tr.device), xd, L_MIN)
    assert torch.equal(_bits(y), _bits(y2))
