"""Per-link power statistics formed on the device (Tracer.power_profiles, hrt_power_profiles,
hermespy_rt.compute_power_profiles) against float64 numpy sums over the same float inputs: Tracer.paths(nonzero_only=
False), Tracer.los() and hrt_launch_dirs_host (the departure direction of a scatter record), as
test_gpu_array_channel.py forms them.

Tolerances per (link, pol): moments <= 1e-9 * sum |term| (u_tx moments: + 2^-22 P for the device's libm); histogram
bins <= (1e-12 + N 2^-61) P with N the link's term count, angle bins plus the power of the terms whose bin coordinate
lies within 1e-6 of a bin edge."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi, power

from . import configs as K
from . import scenes_gen as G
from . import planted as PL
from .pathsum_util import F, _cfg, _tracer
from .pathsum_util import power_check as _check
from .pathsum_util import power_reference as _reference

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _terms(tr, los=True, scatter=True):
    """every term of the trace: link, p [n, 2], tau, nu, u_rx [n, 3], u_tx [n, 3], is_los (float64)"""
    cols = {k: [] for k in ("link", "p", "tau", "nu", "urx", "utx", "los")}
    if scatter:
        P = {k: v.cpu().numpy() for k, v in tr.paths(nonzero_only=False).items()}
        ub = P["unblocked"]
        dirs = PL.launch_dirs(tr).astype(np.float32)
        pw = lambda a: a.real.astype(np.float64) ** 2 + a.imag.astype(np.float64) ** 2   # noqa: E731
        cols["link"].append((P["rx"] * tr.ntx + P["tx"])[ub])
        cols["p"].append(np.stack([pw(P["a_te"][ub]), pw(P["a_tm"][ub])], axis=1))
        cols["tau"].append(P["tau"][ub].astype(np.float64))
        cols["nu"].append(P["freq_shift"][ub].astype(np.float64))
        cols["urx"].append(P["direction_rx"][ub].astype(np.float64))
        cols["utx"].append(dirs[P["path"][ub]].astype(np.float64))
        cols["los"].append(np.zeros(int(ub.sum())))
    if los and tr.shard.rank == 0:
        L = tr.los()
        for rx in range(tr.nrx):
            for tx in range(tr.ntx):
                q = L[rx, tx]
                status = int(q[0:1].view(np.uint32)[0])
                if status == 0:
                    a, tau, nu, u = 1.0, 0.0, 0.0, np.array([-1.0, 0.0, 0.0])
                elif status == 2:
                    a, tau, nu, u = float(q[1]), float(q[2]), float(q[6]), q[3:6].astype(np.float64)
                else:
                    continue
                cols["link"].append(np.array([rx * tr.ntx + tx]))
                cols["p"].append(np.array([[a * a, a * a]]))
                cols["tau"].append(np.array([tau]))
                cols["nu"].append(np.array([nu]))
                cols["urx"].append(-u[None, :])
                cols["utx"].append(u[None, :])
                cols["los"].append(np.ones(1))
    out = {}
    for k, v in cols.items():
        shape = {"p": (0, 2), "urx": (0, 3), "utx": (0, 3)}.get(k, (0,))
        out[k] = np.concatenate(v) if v else np.zeros(shape)
    out["link"] = out["link"].astype(np.int64)
    out["nlinks"] = tr.nrx * tr.ntx
    return out


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


# (scene, rays, [(tau0, dtau, Ld, Nth, Nph)]); dtau 0: the window covers every delay with Ld bins
SPECS = [(0.0, 0.0, 1024, 0, 0), (0.0, 0.0, 300, 7, 13), (1e-7, 2e-9, 1024, 32, 64)]
CASES = [("C1", None), ("TEST_PY", None), ("COINCIDENT", 8000), ("C3", 20000), ("C4_DOPPLER", 4000),
         ("IN_PLANE_canyon", None)]


def _window(T, ld):
    """tau0, dtau of a window of ld bins that covers every delay"""
    lo, hi = (T["tau"].min(), T["tau"].max()) if T["tau"].size else (0.0, 1e-6)
    lo = min(lo, 0.0)
    return lo, max(hi - lo, 1e-9) * (1 + 1e-6) / ld


@pytest.mark.parametrize("name,n", CASES, ids=[c[0] for c in CASES])
def test_power_profiles_match_numpy_over_paths(name, n):
    tr = _tracer(_cfg(name, n))
    tr.trace()
    for parts in ((True, True), (True, False), (False, True)):
        T = _terms(tr, *parts)
        for tau0, dtau, ld, nth, nph in SPECS:
            if dtau == 0.0:
                tau0, dtau = _window(T, ld)
            got = _np(tr.power_profiles(tau0, dtau, ld, nth, nph, los=parts[0], scatter=parts[1]))
            assert got["buffer"].dtype == np.float64 and np.isfinite(got["buffer"]).all()
            _check(got, _reference(T, tau0, dtau, ld, nth, nph), (name, parts, ld, nth, nph))
    tr.close()


def test_closure_and_los_identity():
    """a window over every delay sums to P, both spectra sum to P; P_LOS = |H|^2 of the LoS-only channel"""
    tr = _tracer(K.small(K.C4_DOPPLER, 4000))
    tr.trace()
    T = _terms(tr)
    tau0, dtau = _window(T, 512)
    got = _np(tr.power_profiles(tau0, dtau, 512, 9, 17))
    P = got["moments"][..., abi.POWER_P]
    N = got["moments"][..., abi.POWER_COUNT]
    bound = (1e-12 + N * 2.0 ** -61) * P
    assert (np.abs(got["pdp"].sum(axis=-1) - P) <= bound).all()
    for k in ("arrival", "departure"):
        assert (np.abs(got[k].sum(axis=(-2, -1)) - P) <= bound).all()
    H = tr.channel(3e9, 1e6, 1, scatter=False).cpu().numpy()[..., 0, 0]   # [nrx, ntx, 2]
    pl = got["moments"][..., abi.POWER_P_LOS]
    assert np.allclose(pl, np.abs(H.astype(np.complex128)) ** 2, rtol=1e-6, atol=0)
    assert (pl > 0).any()
    tr.close()


def test_coincident_los_is_unit_power_at_zero_delay():
    tr = _tracer(K.small(K.COINCIDENT, 4000))
    tr.trace()
    m = _np(tr.power_profiles(0.0, 1e-9, 16, 4, 8, scatter=False))
    mo = m["moments"][0, 0]
    assert (mo[:, abi.POWER_COUNT] == 1).all() and (mo[:, abi.POWER_P] == 1).all()
    assert (mo[:, abi.POWER_P_LOS] == 1).all()
    assert (mo[:, abi.POWER_P_TAU] == 0).all() and (mo[:, abi.POWER_P_TAU2] == 0).all()
    assert (m["pdp"][0, 0, :, 0] == 1).all() and m["pdp"][0, 0, :, 1:].sum() == 0
    s = power.summarize(m["moments"])
    assert s["k_factor_db"][0, 0] == np.inf and s["rms_delay_spread_s"][0, 0] == 0
    tr.close()


def test_shards_accumulate_and_determinism():
    import torch
    c = K.small(K.C3, 30000)
    spec = (0.0, 5e-9, 600, 32, 64)
    tr = _tracer(c)
    tr.trace()
    whole = tr.power_profiles(*spec)["buffer"]
    again = tr.power_profiles(*spec)["buffer"]
    assert torch.equal(whole.view(torch.int64), again.view(torch.int64))   # bit-identical
    out = torch.zeros_like(whole)
    tr.power_profiles(*spec, out=out, accumulate=True)
    tr.power_profiles(*spec, out=out, accumulate=True)
    assert torch.equal(out, 2 * whole)
    ref = _reference(_terms(tr), *spec)
    _check(abi.power_views(whole.cpu().numpy(), tr.nrx, tr.ntx, abi.power_spec(*spec)), ref, "whole")
    tr.close()
    for world in (2, 3):
        acc = None
        for r in range(world):
            ts = _tracer(c, rank=r, world=world, chunk=64)
            ts.trace()
            acc = ts.power_profiles(*spec, out=acc, accumulate=acc is not None)["buffer"]
            ts.close()
        # LoS counted once; the fixed-point scales are each shard's own
        _check(abi.power_views(acc.cpu().numpy(), tr.nrx, tr.ntx, abi.power_spec(*spec)), ref, ("shards", world))


_PYBIND_CALL = """import sys
import numpy as np
sys.path.insert(0, {repo!r})
import hermespy_rt_amd
import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
import hermespy_rt
from hermespy_rt_amd import abi, lib
from tests import configs as K
c = K.small(K.C3, 20000)
d = hermespy_rt.compute_power_profiles(c["scene_path"], np.array(c["rx_pos"], np.float32),
                                       np.array(c["tx_pos"], np.float32), np.array(c["rx_vel"], np.float32),
                                       np.array(c["tx_vel"], np.float32), c["f_ghz"], len(c["rx_pos"]),
                                       len(c["tx_pos"]), c["num_paths"], c["num_bounces"], *{spec})
np.save(sys.argv[1], d["buffer"])
assert d["moments"].base is not None and d["arrival"].shape[-2:] == ({spec[3]}, {spec[4]})
st = lib.Stats()
d2 = abi.run_compute_power_profiles(lib.load(), *K.args(c), abi.power_spec(*{spec}), stats=st)
assert np.array_equal(d["buffer"], d2["buffer"])
print("batches", int(st.num_batches))
"""


@pytest.mark.parametrize("batched", [False, True], ids=["one_batch", "batched"])
def test_compute_power_profiles_matches_tracer(tmp_path, batched):
    c = K.small(K.C3, 20000)
    spec = (0.0, 4e-9, 700, 7, 13)
    tr = _tracer(c)
    tr.trace()
    want = _np(tr.power_profiles(*spec))
    ref = _reference(_terms(tr), *spec)
    _check(want, ref, "tracer")
    env = dict(os.environ)
    if batched:   # a budget below one workspace of the whole launch set
        env["HRT_WORKSPACE_BYTES"] = str(int(tr.ws.numel()) * 2 // 3)
    nrx, ntx = tr.nrx, tr.ntx
    tr.close()
    out = tmp_path / "p.npy"
    code = _PYBIND_CALL.format(repo=REPO, spec=spec)
    p = subprocess.run([sys.executable, "-c", code, str(out)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    batches = int(p.stdout.split()[-1])
    assert batches >= 2 if batched else batches == 1
    got = abi.power_views(np.load(out), nrx, ntx, abi.power_spec(*spec))
    _check(got, ref, ("drop-in", batched))


def test_generated_scene_resorted_two_tx(tmp_path):
    """> 1 024 triangles (the live list is re-sorted between bounces) and 2 TX: the TX segments of the hit blocks"""
    p = str(tmp_path / "room.hrt")
    G.room_with_clutter(p, 120, seed=5)
    c = G.cfg(p, [[3.0, 2.0, 1.5], [-5.0, 4.0, 2.0]], [[-10.0, -6.0, 3.0], [12.0, 5.0, 4.0]], 6000, 3,
              tx_vel=[[1.0, 0.0, 0.0], [0.0, -2.0, 0.0]])
    tr = _tracer(c)
    assert tr.num_tri > 1024
    tr.trace()
    T = _terms(tr)
    tau0, dtau = _window(T, 257)
    _check(_np(tr.power_profiles(tau0, dtau, 257, 11, 19)), _reference(T, tau0, dtau, 257, 11, 19), "room")
    tr.close()


def test_eight_by_eight_at_the_largest_grid():
    """C5 endpoints (8 TX x 8 RX), few rays, Ld = 2^16 and Nth x Nph = 2^14: histograms past the LDS budget"""
    c = K.small(K.C5, 256)
    c["num_bounces"] = 2
    tr = _tracer(c)
    tr.trace()
    T = _terms(tr)
    tau0, dtau = _window(T, 1 << 16)
    got = _np(tr.power_profiles(tau0, dtau, 1 << 16, 128, 128))
    assert got["moments"].shape == (8, 8, 2, F) and got["arrival"].shape == (8, 8, 2, 128, 128)
    _check(got, _reference(T, tau0, dtau, 1 << 16, 128, 128), "8x8")
    tr.close()


def test_scratch_too_small_is_refused():
    import torch
    tr = _tracer(K.small(K.C1, 2000))
    tr.trace()
    spec = abi.power_spec(0.0, 1e-9, 64, 4, 4)
    need = C.c_uint64(0)
    assert tr.L.hrt_power_profiles_scratch_bytes(tr.problem, C.byref(tr.shard), C.byref(spec), C.byref(need)) == 0
    scratch = torch.empty(int(need.value), dtype=torch.uint8, device=tr.device)
    out = torch.empty(abi.power_out_doubles(1, 1, spec), dtype=torch.float64, device=tr.device)
    rc = tr.L.hrt_power_profiles(tr.problem, C.byref(tr.shard), C.c_void_p(tr.ws.data_ptr()), C.byref(spec),
                                 C.c_void_p(scratch.data_ptr()), C.c_uint64(int(need.value) - 1),
                                 C.c_void_p(out.data_ptr()), 0, None)
    assert rc == -1 and b"scratch" in tr.L.hrt_last_error()
    tr.close()
