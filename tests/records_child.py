"""The GPU step of tests/test_gpu_records_planted.py, a process of its own (tune switches are latched per process):
python -m tests.records_child JOB.json STATES.npz OUT.npz

For num_bounces = 1 and = 3 (record block 0 and 2) it creates the Tracer of the job's scene and, per list of the job,
fills the workspace with records_util.POISON, plants hit block nb - 1 and counts[nb], runs Tracer.debug_last_launch() and
keeps record block nb - 1, mask block nb - 1, the error word and the number of bytes that changed anywhere the launch
has no business writing.  The route the environment selects (HRT_TUNE) is confirmed from hrt_debug_table_info.  With
"refusals" the entry's refusals are exercised, each with a whole-workspace comparison (nothing launched).  The checks
against the oracle are the parent's."""
import hashlib
import json
import sys
import time

import numpy as np


def main(job_path, states_path, out_path):
    t_start = time.time()
    job = json.load(open(job_path))
    S = dict(np.load(states_path))
    import torch

    from hermespy_rt_amd import abi, device
    from hermespy_rt_amd import lib as hlib

    from . import records_util as RU
    rx = np.asarray(job["rx_pos"], np.float32).reshape(-1, 3)
    tx = np.asarray(job["tx_pos"], np.float32).reshape(-1, 3)
    nrx = rx.shape[0]
    out = dict(lists=np.asarray(job["lists"]))
    poison = int(np.array([RU.POISON], np.uint32).view(np.int32)[0])
    for nb in job["num_bounces"]:
        tr = device.Tracer(job["scene_path"], rx, tx, np.zeros_like(rx), np.zeros_like(tx), job["f_ghz"],
                           job["num_paths"], nb)
        info = abi.debug_table_info(tr.L, tr.problem)
        T, cap, L = tr.num_tri, tr.cap, tr.layout
        assert 64 < T <= 256 and cap >= RU.MASTER_N, (T, cap)
        # the route: patch tables <=> the plan gives launch nb to hrt_records_kernel (a staged one-block flat table)
        if job["route"] == "no_patch":
            assert not (info["kinds"] & abi.CAND_KINDS["patch"]), "no_patch=1 did not take the patch tables away"
        else:
            assert info["kinds"] & abi.CAND_KINDS["patch"], "this problem has no patch tables: not the records kernel's route"
        row_of_flat = np.zeros(T, np.int64)
        row_of_flat[tr.tri_order[:T]] = np.arange(T)
        out.update(tri_order=tr.tri_order[:T].copy(), nuv=info["nuv"], hmax=np.float32(info["hmax"]), cap=cap,
                   kinds=info["kinds"])
        ws32 = tr.ws[:tr.ws.numel() // 4 * 4].view(torch.int32)
        off = {k: int(getattr(L, k)) for k in ("off_counts", "off_los", "off_hits", "off_recs", "off_masks", "off_chunk_cnt")}
        rb = int(L.rec_block_bytes)
        mb = nrx * (cap // 64) * 8
        # bytes the launch may write: the control words behind counts[nb], record and mask block nb - 1, and the scratch
        # behind the mask blocks (chunk counts, shadow results)
        allowed = np.zeros(tr.ws.numel(), bool)
        allowed[off["off_counts"] + 4 * (nb + 1):off["off_los"]] = True
        allowed[off["off_recs"] + (nb - 1) * rb:off["off_recs"] + nb * rb] = True
        allowed[off["off_masks"] + (nb - 1) * mb:off["off_masks"] + nb * mb] = True
        allowed[off["off_chunk_cnt"]:] = True

        def plant(st, n):
            ws32.fill_(poison)
            cnt = tr.counts_tensor()
            cnt[:nb] = 0
            cnt[nb] = n
            assert (st["tri"][:n] < T).all()   # the planted states never leave the table
            blk = np.full((len(hlib.HIT_FIELDS), n), 0, np.int32)
            f = {name: k for k, name in enumerate(hlib.HIT_FIELDS)}
            u = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)   # noqa: E731
            blk[f["ray"]] = np.arange(n, dtype=np.int32)
            blk[f["tri"]] = row_of_flat[st["tri"][:n]].astype(np.int32)
            blk[f["theta"]] = u(st["theta"][:n])
            blk[f["fs0"]] = u(0.5 + np.arange(n, dtype=np.float32))
            for j, c in enumerate("xyz"):
                blk[f["o" + c]] = u(st["o"][:n, j])
                blk[f["d" + c]] = u(st["d"][:n, j])
            for j, name in enumerate(("a_te_re", "a_te_im", "a_tm_re", "a_tm_im")):
                blk[f[name]] = u(st["amp"][:n, j])
            blk[f["tau"]] = u(st["tau"][:n])
            tr.hit_block(nb - 1)[:, :n] = torch.from_numpy(blk).to(tr.device)
            torch.cuda.synchronize(tr.device)

        def state_of(name):
            if name == "replaced":
                return {k[4:]: v for k, v in S.items() if k.startswith("rep_")}, RU.MASTER_N
            if name == "perm":
                return {k: v[RU.PERM] for k, v in S.items() if not k.startswith("rep_")}, RU.MASTER_N
            n = int(name.lstrip("n").split("_")[0])
            return {k: v for k, v in S.items() if not k.startswith("rep_")}, n

        for name in job["lists"]:
            st, n = state_of(name)
            plant(st, n)
            before = tr.ws.cpu().numpy().copy()
            tr.debug_last_launch()
            after = tr.ws.cpu().numpy()
            changed = before != after
            key = "nb%d_%s_" % (nb, name)
            out[key + "rec"] = tr.rec_block(nb - 1).cpu().numpy().view(np.uint32).copy()
            out[key + "mask"] = tr.mask_block(nb - 1).cpu().numpy().view(np.uint32).copy()
            out[key + "err"] = np.uint32(tr.error_word())
            out[key + "changed_outside"] = np.int64((changed & ~allowed).sum())
            out[key + "rest_same_hash"] = (hashlib.sha256(before[~allowed].tobytes()).hexdigest() ==
                                           hashlib.sha256(after[~allowed].tobytes()).hexdigest())
            out[key + "n"] = n
        if job.get("refusals") and nb == max(job["num_bounces"]):
            st, n = state_of("n65")
            refused = []

            def refusal(what, call):
                before = tr.ws.cpu().numpy().copy()
                try:
                    call()
                except RuntimeError as e:
                    assert "(-1)" in str(e), e   # HRT_E_INVALID
                    refused.append(what)
                torch.cuda.synchronize(tr.device)
                assert np.array_equal(before, tr.ws.cpu().numpy()), "%s: the workspace changed (something ran)" % what

            plant(st, n)
            tr.counts_tensor()[nb] = cap + 1
            refusal("counts_beyond_cap", tr.debug_last_launch)
            plant(st, n)
            refusal("short_workspace", lambda: abi.debug_last_launch(tr.L, tr.problem, tr.shard, tr.ws.data_ptr(), tr.ws.numel() - 256))
            refusal("nb_0", lambda: abi.debug_last_launch(tr.L, tr.problem, hlib.Shard(job["num_paths"], 0, 1, 0, 0), tr.ws.data_ptr(), tr.ws.numel()))
            refusal("null_workspace", lambda: abi.debug_last_launch(tr.L, tr.problem, tr.shard, 0, tr.ws.numel()))
            out["refused"] = np.asarray(refused)
        tr.close()
    out["child_seconds"] = time.time() - t_start
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3])
