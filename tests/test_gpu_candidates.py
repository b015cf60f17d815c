"""The candidate-mask tables, lane by lane, on planted rays.

Every kernel that traces a ray on tables of at most 256 triangles takes its candidates from bit masks built once per
problem -- patch tables (hrt_patch_build_kernel; patch_locate / patch_load), the TX cell masks of launch 0
(hrt_txcell_build_kernel; txcell_load) and the per-cell masks on at most 64 triangles (hrt_rxt_build_kernel;
rxt_inside / rxt_cell_load) -- and only survivors of that lookup run the reference's exact sequence.  Bit-exactness of
everything downstream rests on: THE CLOSEST HIT OVER A LANE'S CANDIDATES IS THE CLOSEST HIT OVER THE WHOLE TABLE.  The
hot kernels walk the union of a wave's masks, so the parity tests cannot see a wrong entry; here hrt_debug_candidates
(include/hrt_device.h) returns each lane's OWN words, before any union, for queries planted where the lookup decides
something (tests/candidates_util.py), and the reference is the oracle's full scan (oracle.closest_hits):

  soundness   wherever a lane is served, the scan restricted to its mask equals the full scan in triangle AND distance
              bits (the shadow modes too: the reference carries theta from the shadow winner at any distance);
  serving     every must-serve query is served (100 %: a lookup that serves nobody is trivially sound), every
              must-not-serve query is not, an unserved lane returns zero words, no mask has a bit at or beyond
              num_tri, the patch index lies in its triangle's range and equals iv nu + iu for cell-centre origins;
  controls    on the host: the winner's bit cleared in one downloaded mask is reported as exactly that query.

Every GPU step is a process of its own (tests/candidates_child.py) under a time limit; after a step that failed, none
is started again.  The test prints, per case and mode, the mean and the largest mask population of the served lanes and
the share of whole-table masks (DESIGN_ACCEL.md A.5 keeps the first run's figures); no cap is asserted on them.

The case `canyon_big_offsets` puts the masks of the last apexes beyond byte offset 2^31 (patch_load addresses with
32-bit offsets cast through int): 16.8 M patches x 6 apexes = 2.7 GB of tables; it is the only case of that size.
Measured on an MI355X: the problem with its tables is created in 0.24 s, the case's whole process takes 2.3 s (as
every other case's: starting Python and the HIP runtime is most of it), its lookups 4 ms."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import oracle

from . import candidates_util as CU
from . import configs as K
from .tune import tuned

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 180
BIG_TIMEOUT_S = 300
NO_HIT = 0xFFFFFFFF

_CANYON = K.IN_PLANE["canyon"]
CASES = dict(
    canyon=dict(cfg=_CANYON, modes=[0, 1, 2], refused=[3], all_served=True),
    canyon_coarse=dict(cfg=_CANYON, modes=[0, 1], tune=dict(patch_size=2.0), spread=1),
    canyon_fine=dict(cfg=_CANYON, modes=[0, 1], tune=dict(patch_size=0.2), spread=1),
    canyon_small_budget=dict(cfg=_CANYON, modes=[0, 1], tune=dict(HRT_PATCH_MAX_BYTES="2e7"), spread=1, enlarged=True),
    canyon_big_offsets=dict(cfg=_CANYON, modes=[0, 1], tune=dict(patch_size=0.05, HRT_PATCH_MAX_BYTES="3.4e9"), spread=0,
                            timeout=BIG_TIMEOUT_S, beyond_2g=True),
    c4=dict(cfg=K.C4, modes=[3], refused=[0, 1, 2]),
    c4_no_txt=dict(cfg=K.C4, modes=[3], tune=dict(no_txt=1)),
    c1=dict(cfg=K.C1, modes=[3], refused=[0, 1, 2]),
)
for _name, _g in CU.GENERATED.items():
    CASES[_name] = dict(gen=_g, modes=[0, 1, 2], refused=[3])

_failed = []    # the first GPU step that failed: nothing is started after it
_results = {}   # case -> everything the child wrote plus the oracle's scans (computed once, shared, left unchanged)


def _scene_of(name, tmp):
    case = CASES[name]
    if "gen" in case:
        path = os.path.join(str(tmp), name + ".hrt")
        rx, tx, n_bad = CU.generated_scene(path, **case["gen"])
        return dict(scene_path=path, rx_pos=rx, tx_pos=tx, f_ghz=3.5), n_bad
    c = case["cfg"]
    return dict(scene_path=c["scene_path"], rx_pos=c["rx_pos"], tx_pos=c["tx_pos"], f_ghz=c["f_ghz"]), 0


def result(name, tmp_path_factory):
    """the child's arrays of case `name` plus, per mode, full = closest_hits over all triangles and restricted = the
    scan over each lane's own mask"""
    if name in _results:
        return _results[name]
    if _failed:
        pytest.fail("not started: GPU step %s failed before" % _failed[0])
    case = CASES[name]
    tmp = tmp_path_factory.mktemp("cand_" + name)
    job, n_bad = _scene_of(name, tmp)
    job.update(modes=case["modes"], refused=case.get("refused", []), spread=case.get("spread", 2), seed=11)
    jpath, opath = os.path.join(str(tmp), "case.json"), os.path.join(str(tmp), "out.npz")
    json.dump(job, open(jpath, "w"))
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, "-m", "tests.candidates_child", jpath, opath], cwd=REPO, capture_output=True,
                           text=True, timeout=case.get("timeout", STEP_TIMEOUT_S), env=tuned(**case.get("tune", {})))
    except subprocess.TimeoutExpired:
        _failed.append("%s (time limit)" % name)
        raise
    if p.returncode != 0:
        _failed.append("%s (exit %d)" % (name, p.returncode))
        pytest.fail("%s: exit %d\n%s" % (name, p.returncode, p.stderr[-3000:]))
    R = dict(np.load(opath))
    R["child_seconds"] = time.time() - t0
    R["flat"] = oracle.flatten(oracle.read_hrt(job["scene_path"]))
    R["n_bad"] = n_bad
    T = R["flat"]["tri_vtx"].shape[0]
    R["T"] = T
    inv = np.zeros(T, np.int64)
    inv[R["tri_order"]] = np.arange(T)
    R["row_of_orig"] = inv
    for m in case["modes"]:
        pre = "m%d_" % m
        got = R[pre + "out"]
        R[pre + "served"] = got[:, 0] == 1
        R[pre + "masks"] = CU.words_to_masks(got[:, 2:])
        R[pre + "full"] = oracle.closest_hits(R["flat"], R[pre + "o"], R[pre + "d"])
        R[pre + "restricted"] = oracle.closest_hits(R["flat"], R[pre + "o"], R[pre + "d"], R[pre + "masks"], R["tri_order"])
    print("%s: T %d, %d patches, problem %.2f s, child %.2f s, lookups %s s" % (
        name, T, int(R["num_patch"]), float(R["t_create"]), R["child_seconds"],
        ["%.3f" % float(R["m%d_seconds" % m]) for m in case["modes"]]))
    _results[name] = R
    return R


def _q(R, m):
    pre = "m%d_" % m
    return {k[len(pre):]: v for k, v in R.items() if k.startswith(pre)}


def _table_stats(name, R, m):
    """what the tables contain, as this test's planted lanes see them (uniform over cells, not distributed like hits)"""
    served = R["m%d_served" % m]
    pop = CU.popcount(R["m%d_masks" % m])[served]
    if pop.size:
        print("table contents %s mode %d: %d served lanes, mask population mean %.2f max %d, whole-table masks %.3f %%" % (
            name, m, pop.size, pop.mean(), pop.max(), 100.0 * np.mean(pop == R["T"])))


@pytest.mark.parametrize("name", list(CASES))
def test_soundness(name, tmp_path_factory):
    R = result(name, tmp_path_factory)
    for m in CASES[name]["modes"]:
        q = _q(R, m)
        _table_stats(name, R, m)
        bad = CU.soundness_failures(q["full"], q["restricted"], q["served"])
        assert bad.size == 0, "%s: %d of %d served lanes lose their closest hit, first: %s (restricted scan: flat index %d)" % (
            name, bad.size, int(q["served"].sum()), CU.describe(m, q, bad[0], R["row_of_orig"], q["full"][0]),
            int(q["restricted"][0][bad[0]]))
        assert q["served"].any(), "%s mode %d: nobody was served" % (name, m)
        hits = q["served"] & (q["full"][0] != NO_HIT)
        assert hits.any(), "%s mode %d: no served lane hits anything (the check would be empty)" % (name, m)


@pytest.mark.parametrize("name", list(CASES))
def test_serving(name, tmp_path_factory):
    R = result(name, tmp_path_factory)
    case, T = CASES[name], R["T"]
    assert sorted(R["refused"].tolist()) == sorted(case.get("refused", [])), "modes without a table must be refused"
    for m in case["modes"]:
        q = _q(R, m)
        got, served = q["out"], q["served"]
        assert np.isin(got[:, 0], (0, 1)).all()
        assert not got[~served][:, 1:].any(), "%s mode %d: an unserved lane returned words or a patch index" % (name, m)
        beyond = CU.bits_beyond(q["masks"], T)
        assert beyond.size == 0, "%s mode %d: bits at or beyond num_tri = %d in query %d" % (name, m, T, beyond[0])
    nuv = R["nuv"].astype(np.int64)
    if case.get("all_served"):
        assert (nuv[:, 0] > 0).all(), "every triangle of the canyon is expected to be served: %s are not" % np.flatnonzero(nuv[:, 0] == 0)
    if R["n_bad"]:   # the needles and the triangles without area are the last flat indices
        bad_rows = R["row_of_orig"][T - R["n_bad"]:]
        assert not nuv[bad_rows].any(), "needle / degenerate triangles must come back unserved: %s" % nuv[bad_rows]
        assert (nuv[:, 0] > 0).sum() == T - R["n_bad"]
    if case.get("enlarged"):   # the budget forced bigger cells than the default edge gives: read, not predicted
        assert int(R["num_patch"]) * (R["num_rx"] + R["num_tx"]) * 32 <= 2e7
    if case.get("beyond_2g"):
        assert (int(R["num_rx"]) + int(R["num_tx"]) - 1) * int(R["num_patch"]) * 32 > 2 ** 31, "the last apex's masks do not lie beyond 2^31"
    base = np.concatenate([[0], np.cumsum(nuv[:, 0] * nuv[:, 1])])
    assert base[-1] == int(R["num_patch"])
    for m in (0, 1):
        if m not in case["modes"]:
            continue
        q = _q(R, m)
        served, cls = q["served"], q["cls"]
        plain = np.ones(served.size, bool) if m == 0 else (q["kind"] == CU.IMG_BASE)
        # 100 % of the must-serve class (mode 1: with the unperturbed direction; lines at 0.5 ro_img too)
        must = (cls == CU.MUST) & (plain if m == 0 else (plain | ((q["kind"] == CU.IMG_ROT) & (q["factor"] == 0.5))))
        assert must.sum() > 0
        miss = np.flatnonzero(must & ~served)
        assert miss.size == 0, "%s mode %d: %d of %d must-serve queries are not served, first: row %d cell %s tag %s apex %d" % (
            name, m, miss.size, must.sum(), q["row"][miss[0]], q["cell"][miss[0]], q["tag"][miss[0]], q["apex"][miss[0]])
        never = cls == CU.MUST_NOT
        if m == 1:   # lines that pass the image at 1.1 and 2 ro_img, and the reversed ones
            never |= ((q["kind"] == CU.IMG_ROT) & (q["factor"] > 1.0)) | (q["kind"] == CU.IMG_REV)
        wrong = np.flatnonzero(never & served)
        assert never.sum() > 0 and wrong.size == 0, "%s mode %d: %d queries that must not be served are, first: row %d tag %s" % (
            name, m, wrong.size, q["row"][wrong[0]], q["tag"][wrong[0]])
        for t in ("nan", "row_past") + (("unserved",) if R["n_bad"] else ()):
            assert (q["tag"] == t).any() and not served[q["tag"] == t].any()
        # the patch index: inside the triangle's range; iv nu + iu for cell-centre origins
        r = q["row"][served].astype(np.int64)
        pidx = q["out"][served][:, 1].astype(np.int64)
        assert ((pidx >= base[r]) & (pidx < base[r + 1])).all(), "%s mode %d: a patch index outside its triangle's range" % (name, m)
        c = served & q["centre"]
        assert c.sum() > 0
        rc, cell = q["row"][c].astype(np.int64), q["cell"][c]
        assert np.array_equal(q["out"][c][:, 1].astype(np.int64), base[rc] + cell[:, 1] * nuv[rc, 0] + cell[:, 0])
        # the last cell of a grid and the last apex's table are among the served lanes
        assert (cell[:, 1] * nuv[rc, 0] + cell[:, 0] == nuv[rc, 0] * nuv[rc, 1] - 1).any()
        assert (q["apex"][served] == q["apex"].max()).any()
    if 3 in case["modes"]:
        q = _q(R, 3)
        assert q["inside"].sum() > 0 and q["served"][q["inside"]].all(), "origins inside the region ball must get their cell's mask"
        assert q["outside"].sum() > 0 and not q["served"][q["outside"]].any()
        assert set(np.unique(q["apex"])) == set(range(int(R["num_rx"]) + int(R["num_tx"])))
    if name == "canyon_big_offsets":
        print("canyon_big_offsets: problem %.2f s, child process %.2f s" % (float(R["t_create"]), R["child_seconds"]))


def _control(R, m, pick):
    """clear the winner's bit in the mask of query `pick`: the soundness check must report exactly that query"""
    q = _q(R, m)
    win_row = int(R["row_of_orig"][q["full"][0][pick]])
    assert CU.has_bit(q["masks"][pick:pick + 1], [win_row])[0]
    masks = CU.clear_bit(q["masks"], pick, win_row)
    restricted = oracle.closest_hits(R["flat"], q["o"], q["d"], masks, R["tri_order"])
    bad = CU.soundness_failures(q["full"], restricted, q["served"])
    assert bad.tolist() == [pick], (bad[:10], pick)
    text = CU.describe(m, q, pick, R["row_of_orig"], q["full"][0])
    assert "missing row %d " % win_row in text and "mode %d apex %d" % (m, q["apex"][pick]) in text


def test_negative_controls(tmp_path_factory):
    R = result("gen256", tmp_path_factory)
    q0 = _q(R, 0)
    hit = q0["served"] & (q0["full"][0] != NO_HIT)
    _control(R, 0, int(np.flatnonzero(hit)[0]))
    # a winner at row 255, the last bit of the last word: the first mode that has one
    done = False
    for m in (0, 1, 2):
        q = _q(R, m)
        hit = q["served"] & (q["full"][0] != NO_HIT)
        rows = np.where(hit, R["row_of_orig"][np.minimum(q["full"][0], R["T"] - 1)], -1)
        at255 = np.flatnonzero(rows == 255)
        if at255.size and not done:
            _control(R, m, int(at255[0]))
            done = True
    assert done, "no planted ray is stopped by row 255"
    # the last apex's table: the last TX's image apex
    q1 = _q(R, 1)
    last = q1["served"] & (q1["full"][0] != NO_HIT) & (q1["apex"] == q1["apex"].max())
    _control(R, 1, int(np.flatnonzero(last)[-1]))
    q2 = _q(R, 2)
    last = q2["served"] & (q2["full"][0] != NO_HIT) & (q2["apex"] == q2["apex"].max())
    _control(R, 2, int(np.flatnonzero(last)[-1]))
    R4 = result("c4", tmp_path_factory)
    q3 = _q(R4, 3)
    last = q3["served"] & (q3["full"][0] != NO_HIT) & (q3["apex"] == q3["apex"].max())
    _control(R4, 3, int(np.flatnonzero(last)[-1]))
