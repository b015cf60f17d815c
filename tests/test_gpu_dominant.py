"""The K strongest paths per link selected on the device (Tracer.dominant_paths, hrt_dominant_paths,
hrt_compute_dominant_paths, hermespy_rt.compute_dominant_paths) against the order of include/hermespy_rt.h applied in
numpy (hermespy_rt_amd.dominant) to the same float inputs.  Every comparison is of bytes: the header, every field of
every slot, the zero tail; there is no tolerance anywhere.  Times: profiles/dominant_time.py, DESIGN.md section 15."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi, dominant

from . import configs as K
from . import planted as PL
from .dominant_util import check_bytes, expected, to_numpy, trace_terms
from .pathsum_util import CONFIGS, PARTS, _bits, _cfg, _expect_failure, _force_los_classes, _thin, _traced, _tracer

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, rays, tx kept): the eligible scatter terms per link the CPU oracle gives are in the comments
# The chunk count of a case falls out of its ray count (dm_plan: rays // 512, at most 256): C1's 10 000 rays give 19
# chunks, which is the only reason the merge kernel runs in this file, in two groups of 16 and 3 lists; no case here
# is sized for a merge shape, and none fills the pending slots exactly to 2 048 - K (that takes 1 024 live records
# of a chunk in ascending order).  Those edges, asserted from the chunk plan and a model of the slot rules, are
# tests/test_gpu_dominant_order.py.
CASES = [
    ("C1", None, None),                # 10 000
    ("C3", 20000, None),               # 28 928 .. 29 018
    ("C3", 600, None),                 # 862 .. 864, 1 .. 3 records with a denormal amplitude component
    ("C4_DOPPLER", 2000, 2),           # 822 .. 823, 3 .. 4 of power exactly 0
    ("COINCIDENT", 8000, None),        # 14 785
    ("IN_PLANE_canyon", None, None),   # 8 004 .. 9 369
]
KS = (1, 7, 64, 1024)
FLT_MIN = np.float32(1.17549435e-38)


def _case(name, n, ntx):
    c = dict(_cfg(name, n))
    if ntx:
        c["tx_pos"], c["tx_vel"] = c["tx_pos"][:ntx], c["tx_vel"][:ntx]
    return c


def _denormal(a):
    x = np.abs(np.stack([a.real, a.imag]))
    return ((x > 0) & (x < FLT_MIN)).any(axis=0)


# ------------------------------------------------------------------ 1. traced paths against Tracer.paths()
@pytest.mark.parametrize("name,n,ntx", CASES, ids=["%s_%s" % (c[0], c[1]) for c in CASES])
def test_dominant_paths_match_numpy_over_paths(name, n, ntx):
    tr = _tracer(_case(name, n, ntx))
    tr.trace()
    for parts in PARTS:
        terms = trace_terms(tr, *parts)
        for k in KS:
            got = to_numpy(tr.dominant_paths(k, los=parts[0], scatter=parts[1]))
            want = expected(tr, k, terms=terms)
            check_bytes(got, want, (name, n, parts, k))
            if parts == (True, True) and k == 1024:
                el, kept = want["eligible"].astype(np.int64), got["kept"].astype(np.int64)
                live = np.arange(k) < kept[..., None]
                # the cases must be what they are here for (none of these can pass vacuously)
                if name in ("C1", "C3") and n != 600:
                    assert (el > 1024).any()
                if (name, n) == ("C3", 600):
                    assert ((el > 0) & (el < 1024)).all()
                    assert (live & (_denormal(got["a_te"]) | _denormal(got["a_tm"]))).any()
                if name == "C4_DOPPLER":
                    assert ((el > 0) & (el < 1024)).all()
                    assert ((live & (got["power"] == 0)).sum(axis=-1) >= 2).any()
    tr.close()


# ------------------------------------------------------------------ 2. planted workspaces
def _planted_check(tr, k):
    def check(terms):
        got = to_numpy(tr.dominant_paths(k))
        got["tri"][got["bounce"] >= 0] = 0   # (a planted term list has no triangles: reference() leaves 0 there)
        check_bytes(got, dominant.reference(terms, tr.nrx, tr.ntx, k), ("planted", k))
    return check


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_planted_workspace(name, tmp_path_factory):
    """two power levels per link: the result is decided almost entirely by (bounce, path)"""
    tr, c = _traced(name, tmp_path_factory)
    _force_los_classes(tr)
    counts = tr.counts()
    T = PL.plant(tr)
    assert not PL.design_errors(T)
    for k in (1, 64, 1024):
        check = _planted_check(tr, k)
        check(T)
        # a record dropped or counted twice shows in `eligible` wherever it stands in the order
        for what, i in PL.control_records(T):
            for how in ("drop", "double"):
                with pytest.raises(AssertionError):
                    check(PL.mutate(T, i, how))
    clean = {k: _bits(tr.dominant_paths(k)["buffer"]) for k in (1, 64, 1024)}
    hit = PL.poison(tr, counts, np.float32(3e38))
    assert hit["blocked_records"] + hit["tail_slots"] > 0
    for k, want in clean.items():
        assert tr.torch.equal(_bits(tr.dominant_paths(k)["buffer"]), want), (name, k, "poison read")
    tr.close()


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_planted_workspace_negative_controls(name, tmp_path_factory):
    """A list of K records cannot show a change of a record that is not among them (a swapped polarisation leaves
    the power as it is).  Here the unblocked bits are thinned before planting until every link has fewer than 1024
    eligible terms, so at K = 1024 every planted record is in the list and the check must fail for every
    PL.MUTATIONS x PL.control_records."""
    tr, c = _traced(name, tmp_path_factory)
    _thin(tr, 700)
    T = PL.plant(tr)
    per = np.bincount(PL.link_of(T, tr.ntx), minlength=tr.nrx * tr.ntx)
    assert 0 < per.max() < 1024 and (~T["los"]).sum() > 100
    for k in (1, 64, 1024):
        _planted_check(tr, k)(T)
    _expect_failure(_planted_check(tr, 1024), T, "dominant paths, K = 1024, thinned " + name)
    tr.close()


# ------------------------------------------------------------------ 3. shards, merge, determinism
def test_shards_merge_and_determinism(tmp_path_factory):
    import torch
    c = CONFIGS["C3"](tmp_path_factory)
    for k in (64, 1024):
        tr = _tracer(c)
        tr.trace()
        T = PL.plant(tr, keyed=True)
        first = tr.dominant_paths(k)
        whole = first["buffer"]
        again = tr.dominant_paths(k)["buffer"]
        assert torch.equal(_bits(whole), _bits(again))   # two identical calls: identical bytes
        want = dominant.reference(T, tr.nrx, tr.ntx, k)
        g = to_numpy(first)
        g["tri"][g["bounce"] >= 0] = 0
        check_bytes(g, want, ("keyed whole", k))
        with pytest.raises(ValueError):
            tr.dominant_paths(k, accumulate=True)
        nrx, ntx = tr.nrx, tr.ntx
        tr.close()
        shards = []
        for r in range(3):
            ts = _tracer(c, rank=r, world=3, chunk=64)
            ts.trace()
            PL.plant(ts, keyed=True)
            shards.append(ts)
        for order in ((0, 1, 2), (2, 0, 1)):
            acc = None
            for r in order:
                acc = shards[r].dominant_paths(k, out=acc, accumulate=acc is not None)["buffer"]
            assert torch.equal(_bits(acc), _bits(whole)), (k, order)
        sep = [to_numpy(ts.dominant_paths(k)) for ts in shards]
        assert all(int((s["bounce"] == -1).sum()) == 0 for s in sep[1:])   # only rank 0 has the LoS entries
        host = dominant.merge(dominant.merge(sep[1], sep[2]), sep[0])
        assert np.array_equal(host["buffer"], whole.cpu().numpy()), k
        for ts in shards:
            ts.close()


# ------------------------------------------------------------------ 4. drop-in and module
_DROP_IN_CALL = """import sys
import numpy as np
sys.path.insert(0, {repo!r})
import hermespy_rt_amd
import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
import hermespy_rt
from hermespy_rt_amd import abi, lib
from tests import configs as K
c = K.small(K.C3, 20000)
d = hermespy_rt.compute_dominant_paths(c["scene_path"], np.array(c["rx_pos"], np.float32),
                                       np.array(c["tx_pos"], np.float32), np.array(c["rx_vel"], np.float32),
                                       np.array(c["tx_vel"], np.float32), c["f_ghz"], len(c["rx_pos"]),
                                       len(c["tx_pos"]), c["num_paths"], c["num_bounces"], {k})
np.save(sys.argv[1], d["buffer"])
assert d["power"].base is not None and d["u_tx"].shape == (len(c["rx_pos"]), len(c["tx_pos"]), {k}, 3)
st = lib.Stats()
d2 = abi.run_compute_dominant_paths(lib.load(), *K.args(c), abi.dominant_spec({k}), stats=st)
assert np.array_equal(d["buffer"], d2["buffer"])
for name in d2:
    assert d[name].dtype == d2[name].dtype and d[name].shape == d2[name].shape, name
    assert np.array_equal(np.ascontiguousarray(d[name]).view(np.uint8), np.ascontiguousarray(d2[name]).view(np.uint8)), name
print("batches", int(st.num_batches))
"""


def _flat_to_mesh_face(scene_path):
    """mesh and face of every flat triangle index (the reference's (mesh, face) loop order)"""
    from hermespy_rt_amd import lib
    P = lib.load()
    scene = P.scene_load(str(scene_path).encode())
    try:
        ntri = [int(scene.meshes[i].num_triangles) for i in range(scene.num_meshes)]
    finally:
        abi.free_scene(scene)
    mesh = np.repeat(np.arange(len(ntri)), ntri)
    face = np.concatenate([np.arange(n) for n in ntri])
    return mesh, face


@pytest.mark.parametrize("batched", [False, True], ids=["one_batch", "batched"])
def test_compute_dominant_paths_matches_tracer(tmp_path, batched):
    from hermespy_rt_amd import lib
    c = K.small(K.C3, 20000)
    k = 64
    tr = _tracer(c)
    tr.trace()
    want = to_numpy(tr.dominant_paths(k))
    check_bytes(want, expected(tr, k), "tracer")
    # the host entries report the reference's flat triangle index
    live = want["bounce"] >= 0
    want["tri"][live] = tr.tri_order[want["tri"][live]]
    env = dict(os.environ)
    if batched:   # a budget below one workspace of the whole launch set
        env["HRT_WORKSPACE_BYTES"] = str(int(tr.ws.numel()) * 2 // 3)
    tr.close()
    out = tmp_path / "d.npy"
    p = subprocess.run([sys.executable, "-c", _DROP_IN_CALL.format(repo=REPO, k=k), str(out)], env=env,
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    batches = int(p.stdout.split()[-1])
    assert batches >= 2 if batched else batches == 1
    got = abi.dominant_views(np.load(out), want["kept"].shape[0], want["kept"].shape[1], k)
    check_bytes(got, want, ("drop-in", batched))
    if batched:
        return
    # (mesh, face) of the kept records are those hrt_compute_paths_list reports for the same (rx, tx, bounce, path)
    pl = abi.run_compute_paths_list(lib.load(), *K.args(c))
    mesh, face = _flat_to_mesh_face(c["scene_path"])
    where = {key: i for i, key in enumerate(zip(pl["rx"].tolist(), pl["tx"].tolist(), pl["bounce"].tolist(),
                                                pl["path"].tolist()))}
    checked = 0
    for rx, tx, s in np.argwhere(got["bounce"] >= 0):
        i = where[(int(rx), int(tx), int(got["bounce"][rx, tx, s]), int(got["path"][rx, tx, s]))]
        t = int(got["tri"][rx, tx, s])
        assert (int(mesh[t]), int(face[t])) == (int(pl["mesh"][i]), int(pl["face"][i]))
        assert got["tau"][rx, tx, s] == pl["tau"][i]
        checked += 1
    assert checked >= k


# ------------------------------------------------------------------ 5. edge sizes
def test_link_without_terms_and_los_only():
    tr = _tracer(K.small(K.C3, 4000))
    tr.trace()
    _force_los_classes(tr)
    status = PL.los_status(tr)
    assert (status == 1).any()   # a blocked LoS entry: absent, not counted
    got = to_numpy(tr.dominant_paths(16, los=True, scatter=False))
    check_bytes(got, expected(tr, 16, True, False), "LoS only")
    assert (got["kept"] <= 1).all() and np.array_equal(got["kept"] == 0, status == 1)
    assert np.array_equal(got["kept"], got["eligible"])
    blocked = got["buffer"][16 * tr.nrx * tr.ntx:].reshape(tr.nrx, tr.ntx, -1)[status == 1]
    assert blocked.size and not blocked.any()   # kept = eligible = 0 and an all-zero list
    both = to_numpy(tr.dominant_paths(16))
    check_bytes(both, expected(tr, 16), "blocked LoS with scatter")
    assert not ((both["bounce"] == -1) & (np.arange(16) < both["kept"].astype(np.int64)[..., None]))[status == 1].any()
    tr.close()


def test_eight_by_eight_at_the_largest_list():
    c = K.small(K.C5, 4096)
    c["num_bounces"] = 2
    tr = _tracer(c)
    tr.trace()
    got = to_numpy(tr.dominant_paths(1024))
    assert got["power"].shape == (8, 8, 1024)
    want = expected(tr, 1024)
    rx, tx = 5, 3
    assert int(want["eligible"][rx, tx]) > 0
    for name in ("kept", "eligible") + dominant.FIELDS:
        assert np.array_equal(np.ascontiguousarray(got[name][rx, tx]).view(np.uint8),
                              np.ascontiguousarray(want[name][rx, tx]).view(np.uint8)), name
    check_bytes(got, want, "8x8")
    tr.close()


def test_scratch_too_small_is_refused():
    import torch
    tr = _tracer(K.small(K.C1, 2000))
    tr.trace()
    spec = abi.dominant_spec(64)
    need = C.c_uint64(0)
    assert tr.L.hrt_dominant_paths_scratch_bytes(tr.problem, C.byref(tr.shard), C.byref(spec), C.byref(need)) == 0
    scratch = torch.empty(int(need.value), dtype=torch.uint8, device=tr.device)
    out = torch.empty(abi.dominant_out_bytes(1, 1, spec), dtype=torch.uint8, device=tr.device)
    args = (tr.problem, C.byref(tr.shard), C.c_void_p(tr.ws.data_ptr()), C.byref(spec), C.c_void_p(scratch.data_ptr()))
    rc = tr.L.hrt_dominant_paths(*args, C.c_uint64(int(need.value) - 1), C.c_void_p(out.data_ptr()), 0, None)
    assert rc == -1 and b"scratch" in tr.L.hrt_last_error()
    assert tr.L.hrt_dominant_paths(*args, C.c_uint64(int(need.value)), C.c_void_p(out.data_ptr()), 0, None) == 0
    torch.cuda.synchronize(tr.device)
    with pytest.raises(ValueError):
        tr.dominant_paths(0)
    with pytest.raises(ValueError):
        tr.dominant_paths(1025)
    with pytest.raises(ValueError):
        tr.dominant_paths(4, los=False, scatter=False)
    tr.close()
