"""What the beam taps of a dominant-path list cost: on C3 (4 links, f_s = 122.88 MHz, taps from l_min = 0) with the three
shapes of profiles/beam_taps_time.py -- a 4-element RX ULA x 8 x 8 TX UPA with DFT codebooks of 4 x 16 beams at T = 1,
L = 256 and at T = 64, L = 64, and 16 x 16 by 16 x 16 elements with 8 x 8 beams at L = 512 -- for K = 64 and K = 1 024,
the time of Tracer.sparse_beam_taps on the result of dominant_paths(K), next to three routes timed alternately in the
same run:

    sparse_array_then_torch   Tracer.sparse_array_taps followed by the contraction with the codebooks in torch on the
                              device, where the array taps of the list are accepted (Nr Nt T L <= 2^24)
    torch_alone               the same sum from the list's device views in torch alone (phases in float64, gains, exp,
                              sinc and einsum in float32 / complex64)
    beam_taps                 Tracer.beam_taps on all records of the trace

and how far the list's beam taps are from the whole ones: |h - h_sparse|_F / |h|_F against beam_taps.

    python profiles/sparse_beam_taps_time.py [--reps 3] [--out profiles/sparse/sparse_beam_taps_time.json]

In ONE process: the launch set is traced once; every route has one warm-up call, then `reps` rounds in which the routes
are called one after the other, HIP events around each call, the median reported.  None of the comparisons is a pass
condition."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import hermespy_rt_amd  # noqa: E402,F401
import torch  # noqa: E402  (HIP runtime first, see hermespy_rt_amd.lib)

from hermespy_rt_amd import beams  # noqa: E402
from hermespy_rt_amd import workloads as W  # noqa: E402
from hermespy_rt_amd.device import Tracer  # noqa: E402

FS, L_MIN = 122.88e6, 0
KS = (64, 1024)
C0 = 299792458.0


def ula(n, d, axis):
    e = np.zeros((n, 3), np.float32)
    e[:, axis] = np.arange(n) * d
    return e


def upa(n1, n2, d):
    """n1 x n2 elements in the x-z plane"""
    e = np.zeros((n1 * n2, 3), np.float32)
    e[:, 0] = np.repeat(np.arange(n1), n2) * d
    e[:, 2] = np.tile(np.arange(n2), n1) * d
    return e


def upa_codebook(n1, n2, b1, b2):
    """b1 * b2 beams of an n1 x n2 UPA: Kronecker products of the first b1 / b2 rows of the DFT codebooks"""
    return np.kron(beams.dft_codebook(n1)[:b1], beams.dft_codebook(n2)[:b2]).astype(np.complex64)


def timed_alternately(routes, reps):
    """{name: (median ms, [ms])} of the callables in `routes`: one warm-up call each, then `reps` rounds over all of them"""
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in routes}
    for _ in range(reps):
        for name, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {name: (statistics.median(v), v) for name, v in ms.items()}


def torch_alone(dp, rxe, txe, wrc, wt, fa, fc, l, t):
    """the definition from the list's device views: phases in float64, reduced to a revolution, exp, gains, sinc and
    einsum in float32 / complex64 -> [nrx, ntx, Br, Bt, 2, T, L]; wrc is conj(W_rx)"""
    kept = dp["kept"]
    P = dp["tau"].shape[2]
    live = (torch.arange(P, device=kept.device) < kept[..., None]).to(torch.complex64)
    amp = torch.stack([dp["a_te"], dp["a_tm"]], -1) * live[..., None]                          # [r, t, p, 2]
    tau, nu = dp["tau"].double(), dp["freq_shift"].double()
    ph = nu[..., None] * t - fc * tau[..., None]                                                # [r, t, p, T]
    Wp = torch.polar(torch.ones_like(ph, dtype=torch.float32), (2 * np.pi * (ph - ph.round())).float())
    V = torch.sinc(l - FS * tau[..., None]).float().to(torch.complex64)                         # [r, t, p, L]

    def gains(u, el, w):
        sp = fa / C0 * (u.double() @ el.T)                                                      # [r, t, p, N]
        s = torch.polar(torch.ones_like(sp, dtype=torch.float32), (2 * np.pi * (sp - sp.round())).float())
        return s @ w.T                                                                          # [r, t, p, B]

    U = torch.einsum("rtpa,rtpb,rtpq,rtpm->rtabqmp", gains(dp["u_rx"], rxe, wrc), gains(dp["u_tx"], txe, wt), amp, Wp)
    return U @ V[:, :, None, None, None]                                                        # [r, t, a, b, q, m, L]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    c = W.WORKLOADS[a.config]
    fa = fc = c["f_ghz"] * 1e9
    d = C0 / fa / 2
    tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"], c["num_paths"],
                c["num_bounces"])
    tr.trace()
    small = (ula(4, d, 1), upa(8, 8, d), beams.dft_codebook(4).astype(np.complex64), upa_codebook(8, 8, 4, 4))
    large = (upa(16, 16, d), upa(16, 16, d), upa_codebook(16, 16, 2, 4), upa_codebook(16, 16, 2, 4))
    shapes = (("4x64_4x16_T1_L256", small, 1, 256), ("4x64_4x16_T64_L64", small, 64, 64),
              ("256x256_8x8_T1_L512", large, 1, 512))
    lists = {k: tr.dominant_paths(k) for k in KS}
    rows = []
    for name, (rxe, txe, wr, wt), T, L in shapes:
        dt = 1e-4 if T > 1 else 0.0
        kw = dict(fs=FS, num_taps=L, l_min=L_MIN, dt=dt, num_times=T)
        d_wr, d_wt = torch.from_numpy(wr).to(tr.device), torch.from_numpy(wt).to(tr.device)
        rt, tt = torch.as_tensor(rxe, device=tr.device).double(), torch.as_tensor(txe, device=tr.device).double()
        l = torch.as_tensor(L_MIN + np.arange(L), device=tr.device).double()
        t = torch.as_tensor(dt * np.arange(T), device=tr.device)
        h = tr.beam_taps(rxe, txe, wr, wt, **kw)
        hn = float(torch.linalg.vector_norm(h))
        row = dict(shape=name, config=a.config, Nr=len(rxe), Nt=len(txe), Br=wr.shape[0], Bt=wt.shape[0], L=L, T=T,
                   fs_hz=FS, l_min=L_MIN, links=tr.nrx * tr.ntx)
        for k in KS:
            dp = lists[k]
            r = dict(kept=dp["kept"].cpu().numpy().astype(np.int64).ravel().tolist(),
                     eligible=dp["eligible"].cpu().numpy().astype(np.int64).ravel().tolist())
            hs = tr.sparse_beam_taps(dp, rxe, txe, wr, wt, fc=fc, **kw)
            r["relative_error_to_beam_taps"] = float(torch.linalg.vector_norm(h - hs)) / hn
            routes = {"sparse_beam_taps": lambda: tr.sparse_beam_taps(dp, rxe, txe, wr, wt, fc=fc, out=hs, **kw)}
            try:
                he = tr.sparse_array_taps(dp, rxe, txe, fc=fc, **kw)

                def composed():
                    tr.sparse_array_taps(dp, rxe, txe, fc=fc, out=he, **kw)
                    return torch.einsum("ai,rtijpml,bj->rtabpml", d_wr.conj(), he, d_wt)

                r["relative_difference_to_sparse_array_then_torch"] = float(
                    torch.linalg.vector_norm(composed() - hs) / torch.linalg.vector_norm(hs))
                routes["sparse_array_then_torch"] = composed
            except ValueError as e:
                r["sparse_array_then_torch"] = "refused: %s" % (str(e).splitlines()[0][:200],)
            try:
                ht = torch_alone(dp, rt, tt, d_wr.conj(), d_wt, fa, fc, l, t)
                r["relative_difference_to_torch_alone"] = float(
                    torch.linalg.vector_norm(ht - hs) / torch.linalg.vector_norm(hs))
                del ht
                routes["torch_alone"] = lambda: torch_alone(dp, rt, tt, d_wr.conj(), d_wt, fa, fc, l, t)
            except Exception as e:   # (out of memory at the largest shape, or an operator this build lacks)
                r["torch_alone"] = "unavailable: %s" % (str(e).splitlines()[0][:200],)
            routes["beam_taps"] = lambda: tr.beam_taps(rxe, txe, wr, wt, out=h, **kw)
            for route, (med, every) in timed_alternately(routes, a.reps).items():
                r[route + "_ms"], r[route + "_ms_all"] = med, every
            row["K%d" % k] = r
            del hs, routes
            torch.cuda.empty_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
        del h
        torch.cuda.empty_cache()
    tr.close()
    try:
        commit = subprocess.check_output(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], text=True,
                                         stderr=subprocess.DEVNULL).strip()
    except Exception:
        commit = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(dict(device="MI355X", commit=commit, reps=a.reps, results=rows), fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
