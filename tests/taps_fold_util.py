"""What tests/test_gpu_taps_fold.py compares with tests/golden/taps_fold.json: the scratch sizes of the three taps
families (the host plan: hrt_taps_scratch_bytes, hrt_array_taps_scratch_bytes, hrt_beam_taps_scratch_bytes) and the
sha256 of the raw output bytes of Tracer.taps, array_taps and beam_taps on a planted workspace (tests/planted.py).

The golden file holds what a build of the commit before the taps fold gave (csrc/hrt_taps_gemm.inc,
csrc/hrt_beam_gains.inc, taps_grid() of csrc/host/channel.c).  It is written by hand, on a machine with a GPU:

    python -m tests.taps_fold_util record OUT.json

(HRT_LIB_DIR selects the build.)  Run twice in separate processes on that build, the two files were byte-identical:
the kernels use no float atomics and add the record chunks in a fixed order, so every case repeats and none is left
out.

Plan cases.  The scratch queries read the problem, the shard and the spec, no workspace: the shard handed to them has
SHARD_PATHS rays whatever the tracer traced, so that the 512-record floor of ps_chunks allows 2048 chunks (4096 on one
shard) and the chunk count is ceil(2048 / (links * rblocks * cblocks)): the groups term.  Rows: 4 and 12 / 13 (the form
switch, rtiles 3 / 4), 64 / 65 (rblocks 1 / 2 in the rt = 4 form of the array and beam families; 16 / 17 for the plain
family, whose blocks are 4 row tiles).  Taps: 16 / 17 (ctiles 1 / 2), 64 / 65 (cblocks 1 / 2 at rt = 4), 256 / 257
(cblocks 1 / 2 at rt = 1).  Every combination of these with the three parts and one shard or the second of two.

Output cases.  Shapes, the smallest that reach each form with 17 taps (two column tiles, the second one ragged):
    taps        T = 4 (rt = 1), T = 13 (rt = 4)
    array taps  2 x 1 elements, T = 2 (4 rows, rt = 1); 13 x 1 elements, T = 1 (13 rows, rt = 4)
    beam taps   Bt = 3: 5 x 3 beams, T = 5 (75 rows, rt = 4: the second block of 64 rows begins inside pair 12 and
                the last pair ends inside it); 1 x 3 beams, T = 3 (9 rows, rt = 1: every block of 4 rows after the
                first begins inside a pair).  With Bt = 3 and T = 5 the grid has at least 15 rows, which is the rt = 4
                form, so the rt = 1 case takes T = 3.
Each with and without the LoS part, written plainly and then accumulated once into the same tensor.  The sampling rate
and the carrier are off the planted grid, so the sinc weights and the phases are general."""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

import numpy as np

from hermespy_rt_amd import abi, lib

from . import beam_util as BU
from . import configs as K
from . import planted as PL
from .pathsum_util import _lam, _random, _tracer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "taps_fold.json")
CFG = K.small(K.C3, 2000)   # about 3 000 records per link, several record chunks
SHARD_PATHS = 1 << 22

# (Nr or Br, Nt or Bt, T) by rows of the array and beam families; the plain family has T = rows
PAIR_ROWS = {4: (2, 1, 2), 12: (2, 3, 2), 13: (13, 1, 1), 64: (4, 4, 4), 65: (5, 13, 1)}
PLAIN_ROWS = (4, 12, 13, 16, 17, 64, 65)
TAPS = (16, 17, 64, 65, 256, 257)
PARTS = {"los": (True, False), "scatter": (False, True), "both": (True, True)}
SHARDS = {"1of1": (0, 1), "2of2": (1, 2)}


def _up(n):
    return (n + 255) // 256 * 256


def plan_cases():
    """(key, family, (n1, n2, T), L, parts name, shard name) of every plan case"""
    for fam in ("taps", "array_taps", "beam_taps"):
        rows = PLAIN_ROWS if fam == "taps" else tuple(PAIR_ROWS)
        for r, L, parts, shard in itertools.product(rows, TAPS, PARTS, SHARDS):
            shape = (1, 1, r) if fam == "taps" else PAIR_ROWS[r]
            yield "%s rows%d L%d %s %s" % (fam, r, L, parts, shard), fam, shape, L, parts, shard


def scratch_bytes(tr, fam, shape, L, parts, shard):
    """the scratch size of one plan case and the record chunks it holds (seg, then the partial sums of every chunk,
    then, in the beam family, the LoS gains: csrc/host/channel.c)"""
    n1, n2, T = shape
    los, scatter = PARTS[parts]
    rank, count = SHARDS[shard]
    s = lib.Shard(SHARD_PATHS, rank, count, 0, tr.nb)
    spec = abi.taps_spec(PL.FS, L, -3, PL.FC, 0.0, PL.DT, T, los, scatter)
    buf = np.zeros(16, np.float32)   # (the pointers are tested for NULL only)
    arr = abi.ArraySpec(n1, n2, buf.ctypes.data, buf.ctypes.data, 3e9)
    bm = abi.BeamSpec(n1, n2, buf.ctypes.data, buf.ctypes.data)
    extra = {"taps": (), "array_taps": (C.byref(arr),), "beam_taps": (C.byref(arr), C.byref(bm))}[fam]
    need = C.c_uint64(0)
    rc = getattr(tr.L, "hrt_%s_scratch_bytes" % fam)(tr.problem, C.byref(s), C.byref(spec), *extra, C.byref(need))
    assert rc == 0, (fam, shape, L, parts, shard, tr.L.hrt_last_error().decode())
    links = tr.nrx * tr.ntx
    per = links * 2 * n1 * n2 * T * L * 8
    rest = need.value - _up(tr.nb * (tr.ntx + 1) * 4)
    if fam == "beam_taps":
        rest -= _up(links * n1 * n2 * 8)
        n = rest // per
        assert _up(n * per) == rest, (need.value, per, rest)
    else:
        n = rest // per
        assert n * per == rest, (need.value, per, rest)
    return need.value, n


def plan_sizes(tr):
    return {key: scratch_bytes(tr, *case)[0] for key, *case in plan_cases()}


# ------------------------------------------------------------------ output bytes
FS_OUT, FC_OUT = PL.FS * 1.37, PL.FC * 1.013
OUT_TAPS, OUT_LMIN, OUT_T0 = 17, -3, 3.0 * PL.DT
OUT_SHAPES = {"taps": {1: (1, 1, 4), 4: (1, 1, 13)},
              "array_taps": {1: (2, 1, 2), 4: (13, 1, 1)},
              "beam_taps": {1: (1, 3, 3), 4: (5, 3, 5)}}


def output_cases():
    for fam, forms in OUT_SHAPES.items():
        for rt, los in itertools.product(forms, (True, False)):
            yield "%s rt%d %s" % (fam, rt, "both" if los else "scatter"), fam, forms[rt], los


def _sha(x):
    b = x.detach().cpu().numpy().view(np.uint8)
    return hashlib.sha256(b.tobytes()).hexdigest()


def output_hashes(tr, fam, shape, los):
    """(sha256 of the output written plainly, sha256 after the same call accumulated into it once)"""
    n1, n2, T = shape
    lam = _lam(CFG)
    kw = dict(fc=FC_OUT, t0=OUT_T0, dt=PL.DT, num_times=T, los=los, scatter=True)
    if fam == "taps":
        call = lambda **o: tr.taps(FS_OUT, OUT_TAPS, OUT_LMIN, **kw, **o)   # noqa: E731
    elif fam == "array_taps":
        rxe, txe = _random(n1, 2 * lam, 31), _random(n2, 2 * lam, 32)
        call = lambda **o: tr.array_taps(rxe, txe, FS_OUT, OUT_TAPS, OUT_LMIN, **kw, **o)   # noqa: E731
    else:
        rxe, txe = _random(37, 2 * lam, 33), _random(5, 2 * lam, 34)   # 37 elements: two element tiles, one ragged
        wr, wt = BU.random_weights(n1, 37, 35), BU.random_weights(n2, 5, 36)
        call = lambda **o: tr.beam_taps(rxe, txe, wr, wt, FS_OUT, OUT_TAPS, OUT_LMIN, **kw, **o)   # noqa: E731
    out = call()
    tr.torch.cuda.synchronize(tr.device)
    first = _sha(out)
    call(out=out, accumulate=True)
    tr.torch.cuda.synchronize(tr.device)
    return first, _sha(out)


def planted_tracer():
    tr = _tracer(CFG)
    tr.trace()
    T = PL.plant(tr)
    assert not PL.design_errors(T), PL.design_errors(T)
    return tr


def record(path):
    tr = planted_tracer()
    out = {"scratch_bytes": plan_sizes(tr), "sha256": {}}
    for key, fam, shape, los in output_cases():
        out["sha256"][key], out["sha256"][key + " accumulated"] = output_hashes(tr, fam, shape, los)
    tr.close()
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "record":
        sys.exit("usage: python -m tests.taps_fold_util record OUT.json")
    record(sys.argv[2])
