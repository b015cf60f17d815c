"""What the beam channel of a dominant-path list costs: on C3 (4 links, 1 024 subcarriers at 30 kHz around the carrier)
with the three shapes of profiles/beam_channel_time.py -- a 4-element RX ULA x 8 x 8 TX UPA with DFT codebooks of 4 x 16
beams at T = 1 and at T = 14, and 16 x 16 by 16 x 16 elements with 8 x 8 beams -- for K = 64 and K = 1 024, the time
of Tracer.sparse_beam_channel on the result of dominant_paths(K), next to three baselines measured in the same run:

    beam_channel              Tracer.beam_channel on all records of the trace
    sparse_array_then_torch   Tracer.sparse_array_channel followed by the contraction with the codebooks in torch on the
                              device, where the array channel of the list is accepted (Nr Nt T K_f <= 2^24)
    torch_alone               the same sum from the list's device views in torch alone (phases in float64, gains,
                              exp and einsum in complex64)

and how far the list's beam channel is from the whole one: |B - B_sparse|_F / |B|_F against beam_channel.

    python profiles/sparse_beam_channel_time.py [--reps 3] [--out profiles/sparse/sparse_beam_channel_time.json]

In ONE process: the launch set is traced once; every route has one warm-up call, then HIP events around each of `reps`
calls, the median reported.  None of the comparisons is a pass condition."""
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

KF, DF = 1024, 30e3
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


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms


def torch_alone(dp, rxe, txe, wrc, wt, fa, f, t):
    """the definition from the list's device views: phases in float64, reduced to a revolution, exp, gains and einsum
    in complex64 -> [nrx, ntx, Br, Bt, 2, T, K]; wrc is conj(W_rx)"""
    kept = dp["kept"]
    P = dp["tau"].shape[2]
    live = (torch.arange(P, device=kept.device) < kept[..., None]).to(torch.complex64)
    amp = torch.stack([dp["a_te"], dp["a_tm"]], -1) * live[..., None]                          # [r, t, p, 2]
    tau, nu = dp["tau"].double(), dp["freq_shift"].double()
    ph = nu[..., None, None] * t[:, None] - f[None, :] * tau[..., None, None]                   # [r, t, p, T, K]
    Wp = torch.polar(torch.ones_like(ph, dtype=torch.float32), (2 * np.pi * (ph - ph.round())).float())

    def gains(u, el, w):
        sp = fa / C0 * (u.double() @ el.T)                                                      # [r, t, p, N]
        s = torch.polar(torch.ones_like(sp, dtype=torch.float32), (2 * np.pi * (sp - sp.round())).float())
        return s @ w.T                                                                          # [r, t, p, B]

    return torch.einsum("rtpa,rtpb,rtpq,rtpmk->rtabqmk", gains(dp["u_rx"], rxe, wrc), gains(dp["u_tx"], txe, wt),
                        amp, Wp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    c = W.WORKLOADS[a.config]
    fa = c["f_ghz"] * 1e9
    d = C0 / fa / 2
    f0 = fa - (KF // 2) * DF
    tr = Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"], c["num_paths"],
                c["num_bounces"])
    tr.trace()
    small = (ula(4, d, 1), upa(8, 8, d), beams.dft_codebook(4).astype(np.complex64), upa_codebook(8, 8, 4, 4))
    large = (upa(16, 16, d), upa(16, 16, d), upa_codebook(16, 16, 2, 4), upa_codebook(16, 16, 2, 4))
    shapes = (("4x64_4x16_T1", small, 1), ("4x64_4x16_T14", small, 14), ("256x256_8x8_T1", large, 1))
    lists = {k: tr.dominant_paths(k) for k in KS}
    rows = []
    for name, (rxe, txe, wr, wt), T in shapes:
        dt = 1e-3 if T > 1 else 0.0
        d_wr, d_wt = torch.from_numpy(wr).to(tr.device), torch.from_numpy(wt).to(tr.device)
        rt, tt = torch.as_tensor(rxe, device=tr.device).double(), torch.as_tensor(txe, device=tr.device).double()
        f = torch.as_tensor(f0 + DF * np.arange(KF), device=tr.device)
        t = torch.as_tensor(dt * np.arange(T), device=tr.device)
        B = tr.beam_channel(rxe, txe, wr, wt, f0, DF, KF, dt=dt, num_times=T)
        row = dict(shape=name, config=a.config, Nr=len(rxe), Nt=len(txe), Br=wr.shape[0], Bt=wt.shape[0], K_f=KF, T=T,
                   links=tr.nrx * tr.ntx)
        row["beam_channel_ms"], row["beam_channel_ms_all"] = timed(
            lambda: tr.beam_channel(rxe, txe, wr, wt, f0, DF, KF, dt=dt, num_times=T, out=B), a.reps)
        bn = float(torch.linalg.vector_norm(B))
        for k in KS:
            dp = lists[k]
            r = dict(kept=dp["kept"].cpu().numpy().astype(np.int64).ravel().tolist(),
                     eligible=dp["eligible"].cpu().numpy().astype(np.int64).ravel().tolist())
            Bs = tr.sparse_beam_channel(dp, rxe, txe, wr, wt, f0, DF, KF, dt=dt, num_times=T)
            r["sparse_beam_channel_ms"], r["sparse_beam_channel_ms_all"] = timed(
                lambda: tr.sparse_beam_channel(dp, rxe, txe, wr, wt, f0, DF, KF, dt=dt, num_times=T, out=Bs), a.reps)
            r["relative_error_to_beam_channel"] = float(torch.linalg.vector_norm(B - Bs)) / bn
            try:
                H = tr.sparse_array_channel(dp, rxe, txe, f0, DF, KF, dt=dt, num_times=T)

                def route():
                    tr.sparse_array_channel(dp, rxe, txe, f0, DF, KF, dt=dt, num_times=T, out=H)
                    return torch.einsum("ai,rtijpmk,bj->rtabpmk", d_wr.conj(), H, d_wt)

                r["sparse_array_then_torch_ms"], r["sparse_array_then_torch_ms_all"] = timed(route, a.reps)
                r["relative_difference_to_sparse_array_then_torch"] = float(
                    torch.linalg.vector_norm(route() - Bs) / torch.linalg.vector_norm(Bs))
                del H
            except ValueError as e:
                r["sparse_array_then_torch"] = "refused: %s" % (str(e).splitlines()[0][:200],)
            try:
                Bt_ = torch_alone(dp, rt, tt, d_wr.conj(), d_wt, fa, f, t)
                r["torch_alone_ms"], r["torch_alone_ms_all"] = timed(
                    lambda: torch_alone(dp, rt, tt, d_wr.conj(), d_wt, fa, f, t), a.reps)
                r["relative_difference_to_torch_alone"] = float(
                    torch.linalg.vector_norm(Bt_ - Bs) / torch.linalg.vector_norm(Bs))
                del Bt_
            except Exception as e:   # (out of memory at the largest shape, or an operator this build lacks)
                r["torch_alone"] = "unavailable: %s" % (str(e).splitlines()[0][:200],)
            row["K%d" % k] = r
            del Bs
            torch.cuda.empty_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
        del B
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
