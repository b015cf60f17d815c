"""The patch masks built from the patch-to-apex pencil (csrc/hrt_kernels.hip pencil_culls; DESIGN_ACCEL.md A.5 items 4-6),
lane by lane, on rays planted where the new bounds are tightest.

The property is the one of tests/test_gpu_candidates.py: WHEREVER A LANE IS SERVED, THE CLOSEST HIT OVER ITS OWN CANDIDATES
IS THE CLOSEST HIT OVER THE WHOLE TABLE, in triangle and distance bits (the oracle's full scan, oracle.closest_hits) -- the
shadow rays at any distance beyond the RX, the mirrored rays for image apexes.  Planted (tests/candidates_pencil_child.py):
the 8 corners and 12 edge midpoints of a cell's prism at the served limits (1 / 64 cell outside the grid, |h| = hmax - 1e-5),
cells seen at under 2 degrees from the RX, pencils that pass within 1 mm either side of a small triangle's edges and
vertices before and beyond the RX, RXs in triangle planes (the canyon's endpoints; an added RX in the generated scenes),
image lines at 0.9 x ro_img.  Scenes: generated tables of 65 (the smallest with patch tables) and 256 triangles, the canyon
at patch_size 0.5 and 2.0.

test_subset_of_cone: the same queries against tables built with HRT_TUNE patch_cone_only=1 (a child process of its own):
every word is a subset of the cone-only word, the same lanes are served, and on the canyon the mean population is
strictly smaller.

Every GPU step is a process of its own under a time limit; after a step that failed, none is started again."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle

from . import candidates_util as CU
from . import configs as K
from .tune import tuned

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 180
NO_HIT = 0xFFFFFFFF

_CANYON = K.IN_PLANE["canyon"]
CASES = dict(
    gen65=dict(gen=dict(n_tri=65, seed=5, tilt=True)),
    gen256=dict(gen=dict(n_tri=256, seed=8)),
    canyon=dict(cfg=_CANYON, tune=dict(patch_size=0.5)),
    canyon_coarse=dict(cfg=_CANYON, tune=dict(patch_size=2.0)),
)

_failed = []
_results = {}


def _job(name, tmp):
    case = CASES[name]
    if "gen" in case:
        path = os.path.join(str(tmp), name + ".hrt")
        rx, tx, _ = CU.generated_scene(path, **case["gen"])
        # an RX in the plane of the table's first triangle, beside it
        t = oracle.flatten(oracle.read_hrt(path))["tri_vtx"].reshape(-1, 3, 3)[0].astype(np.float64)
        rx = rx + [(t[0] + 1.5 * (t[1] - t[0]) - 0.7 * (t[2] - t[0])).astype(np.float32).tolist()]
        return dict(scene_path=path, rx_pos=rx, tx_pos=tx, f_ghz=3.5)
    c = case["cfg"]
    return dict(scene_path=c["scene_path"], rx_pos=c["rx_pos"], tx_pos=c["tx_pos"], f_ghz=c["f_ghz"])


def _child(name, tmp, key, **tune):
    if _failed:
        pytest.fail("not started: GPU step %s failed before" % _failed[0])
    job = _job(name, tmp)
    jpath, opath = os.path.join(str(tmp), key + ".json"), os.path.join(str(tmp), key + ".npz")
    json.dump(job, open(jpath, "w"))
    try:
        p = subprocess.run([sys.executable, "-m", "tests.candidates_pencil_child", jpath, opath], cwd=REPO, capture_output=True,
                           text=True, timeout=STEP_TIMEOUT_S, env=tuned(**tune))
    except subprocess.TimeoutExpired:
        _failed.append("%s/%s (time limit)" % (name, key))
        raise
    if p.returncode != 0:
        _failed.append("%s/%s (exit %d)" % (name, key, p.returncode))
        pytest.fail("%s/%s: exit %d\n%s" % (name, key, p.returncode, p.stderr[-3000:]))
    R = dict(np.load(opath))
    R["job"] = job
    return R


def result(name, tmp_path_factory):
    if name in _results:
        return _results[name]
    tmp = tmp_path_factory.mktemp("pencil_" + name)
    R = _child(name, tmp, "new", **CASES[name].get("tune", {}))
    R["tmp"] = tmp
    R["flat"] = oracle.flatten(oracle.read_hrt(R["job"]["scene_path"]))
    T = R["flat"]["tri_vtx"].shape[0]
    inv = np.zeros(T, np.int64)
    inv[R["tri_order"]] = np.arange(T)
    R["row_of_orig"], R["T"] = inv, T
    for m in (0, 1):
        pre = "m%d_" % m
        R[pre + "served"] = R[pre + "out"][:, 0] == 1
        R[pre + "masks"] = CU.words_to_masks(R[pre + "out"][:, 2:])
        R[pre + "full"] = oracle.closest_hits(R["flat"], R[pre + "o"], R[pre + "d"])
        R[pre + "restricted"] = oracle.closest_hits(R["flat"], R[pre + "o"], R[pre + "d"], R[pre + "masks"], R["tri_order"])
    _results[name] = R
    return R


def _q(R, m):
    pre = "m%d_" % m
    return {k[len(pre):]: v for k, v in R.items() if k.startswith(pre)}


@pytest.mark.parametrize("name", list(CASES))
def test_soundness_on_planted_pencils(name, tmp_path_factory):
    R = result(name, tmp_path_factory)
    for m in (0, 1):
        q = _q(R, m)
        served = q["served"]
        pop = CU.popcount(q["masks"])
        for t in np.unique(q["tag"]):
            s = served & (q["tag"] == t)
            print("%s mode %d %-12s %5d queries, %5d served, %5d of them hit something, mask population mean %.2f max %d" % (
                name, m, t, int((q["tag"] == t).sum()), int(s.sum()), int((s & (q["full"][0] != NO_HIT)).sum()),
                pop[s].mean() if s.any() else 0.0, pop[s].max() if s.any() else 0))
        bad = CU.soundness_failures(q["full"], q["restricted"], served)
        assert bad.size == 0, "%s: %d of %d served lanes lose their closest hit, first: %s (restricted scan: flat index %d)" % (
            name, bad.size, int(served.sum()), CU.describe(m, q, bad[0], R["row_of_orig"], q["full"][0]), int(q["restricted"][0][bad[0]]))
        assert CU.bits_beyond(q["masks"], R["T"]).size == 0
        # the planted classes are there, served, and stopped by something (the check is not empty)
        tags = ("corner", "graze", "edge_before", "edge_beyond") if m == 0 else ("corner", "graze")
        for t in tags:
            s = served & (q["tag"] == t)
            assert s.any(), "%s mode %d: no %s query is served" % (name, m, t)
            assert (s & (q["full"][0] != NO_HIT)).any(), "%s mode %d: no served %s query hits anything" % (name, m, t)
        # the served limits: every must-serve query IS served (mode 1: the unperturbed line and the lines at 0.5 ro_img)
        must = q["cls"] == CU.MUST
        if m == 1:
            must &= (q["kind"] == CU.IMG_BASE) | ((q["kind"] == CU.IMG_ROT) & (q["factor"] == 0.5))
            at09 = served & (q["kind"] == CU.IMG_ROT) & (q["factor"] == 0.9)
            assert at09.any(), "%s: no image line at 0.9 ro_img is served" % name
        corner = must & (q["tag"] == "corner")
        assert corner.any(), "no corner query is in the must-serve class"
        miss = np.flatnonzero(must & ~served)
        assert miss.size == 0, "%s mode %d: %d must-serve queries are not served, first row %d tag %s" % (
            name, m, miss.size, q["row"][miss[0]], q["tag"][miss[0]])


@pytest.mark.parametrize("name", ["canyon", "gen256"])
def test_subset_of_cone(name, tmp_path_factory):
    R = result(name, tmp_path_factory)
    tune = dict(CASES[name].get("tune", {}), patch_cone_only=1)
    O = _child(name, R["tmp"], "cone", **tune)
    for m in (0, 1):
        pre = "m%d_" % m
        assert np.array_equal(O[pre + "o"], R[pre + "o"]) and np.array_equal(O[pre + "row"], R[pre + "row"])
        served_old = O[pre + "out"][:, 0] == 1
        assert np.array_equal(served_old, R[pre + "served"]), "the builder changes who is served"
        old, new = CU.words_to_masks(O[pre + "out"][:, 2:]), R[pre + "masks"]
        extra = np.flatnonzero((new & ~old).any(axis=1))
        assert extra.size == 0, "%s mode %d: query %d has a bit the cone-only mask lacks" % (name, m, extra[0])
        s = R[pre + "served"]
        p_old, p_new = CU.popcount(old)[s].mean(), CU.popcount(new)[s].mean()
        print("%s mode %d: mean mask population of the served lanes, cone only %.3f, with the pencil %.3f" % (name, m, p_old, p_new))
        if name == "canyon":
            assert p_new < p_old, "the pencil removes nothing on the canyon (%.3f against %.3f)" % (p_new, p_old)
