"""Launch 0 on patch tables as its own instantiation of hrt_fused_kernel (TXCELL: its own LDS image, the reference-order
and material words in it where a seventh of a CU holds them) on whole scenes: the product through the C
ABI against the CPU port (oracle.compute_paths), every output array, the live-list lengths and the LoS block bit for
bit.

Scenes: the street canyon (234 triangles) and gen65 -- words in --, gen256 -- words out.  One RX and one bounce unless
the case says otherwise.  Per scene:

  r1000     1 000 rays: a short list, one packet per wave, a partial last wave
  r65537    65 537 rays: one packet per wave, 257 chunks, four group-closing chunks, a last chunk of one entry
  r262145   262 145 rays: the first count past the short list, four packets per wave, 257 macro-chunks, the last of one ray
  tx2       2 TXs at 1 000 rays: a wave straddles both
  tx65      65 TXs at 300 rays: a TX beyond the image's TX slots

and the canyon once with 4 RXs and 3 bounces at 20 000 rays, so that launches 1 to 3 consume the list launch 0 wrote;
and `tie` at 65 537 rays: a generated room of 116 triangles whose walls are given TWICE, the copy as a mesh of another
material, so that every hit on a wall is an exact tie which the reference-order words of the image decide (with those
words shifted by one row the other cases all pass; the canyon is of one material throughout, so the material words
are judged by gen65 and by this case).
Each case is a process of its own (tests/launch0_patch_child.py) under a time limit; it asserts that no kernel was
switched off (hrt_fallback_state() == 0; an error word that is not clean fails the call itself), so that what was
compared is the fused launch 0 and not the per-launch kernels."""
import os
import subprocess
import sys

import pytest

from tests import configs as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 120
SCENES = {"canyon": (234, True), "gen65": (65, True), "gen256": (256, False)}   # triangles, the words are in
SHAPES = {"r1000": (1, 1000), "r65537": (1, 65537), "r262145": (1, 262145), "tx2": (2, 1000), "tx65": (65, 300)}
CASES = ["%s-%s" % (s, k) for s in SCENES for k in SHAPES] + ["canyon-deep", "tie-r65537"]
TIE_TRI = 128   # 116 generated + the room's 12 once more


def tx_positions(base, n):
    """n TX positions: the case's own first, the others spread on a small lattice around it (all inside the scene)"""
    out = []
    for i in range(n):
        out.append([base[0] + 0.37 * (i % 5), base[1] + 0.29 * ((i // 5) % 5), base[2] + 0.11 * (i // 25)])
    return out


def case_config(name, tmp):
    scene, shape = name.split("-")
    if scene == "canyon":
        c = dict(K.small(K.C3, 1000))
        base_tx, rx = list(c["tx_pos"][0]), [list(p) for p in c["rx_pos"]]
        path = c["scene_path"]
        f = c["f_ghz"]
    elif scene == "tie":
        from oracle.oracle import read_hrt
        from tests import scenes_gen as G0
        from tests.candidates_util import GEN_TX, generated_scene
        path = os.path.join(str(tmp), "tie.hrt")
        rx, _, _ = generated_scene(path, n_tri=TIE_TRI - 12, seed=11)
        meshes = [dict(vs=m["vs"], idx=m["idx"], material_index=m["material_index"], velocity=m["velocity"])
                  for m in read_hrt(path)]
        room = meshes[0]
        assert len(room["idx"]) == 12
        meshes.append(dict(vs=room["vs"].copy(), idx=room["idx"].copy(), material_index=9, velocity=[0, 0, 0]))
        G0.write_hrt(path, meshes)
        base_tx, f = GEN_TX[0], 3.5
    else:
        from tests.candidates_util import GEN_TX, GENERATED, generated_scene
        key = {"gen65": "gen65_tilt", "gen256": "gen256"}[scene]
        path = os.path.join(str(tmp), scene + ".hrt")
        rx, _, _ = generated_scene(path, **GENERATED[key])
        base_tx, f = GEN_TX[0], 3.5
    from tests import scenes_gen as G
    if shape == "deep":
        rx4 = (rx * 4)[:4] if len(rx) < 4 else rx[:4]
        rx4 = [[p[0] + 0.5 * i, p[1], p[2]] for i, p in enumerate(rx4)]
        return G.cfg(path, rx4, [base_tx], 20000, 3, f=f)
    ntx, rays = SHAPES[shape]
    return G.cfg(path, rx[:1], tx_positions(base_tx, ntx), rays, 1, f=f)


def test_the_cases_are_what_they_are_named_for(tmp_path):
    """No GPU: the tables' sizes, the shapes' chunk arithmetic, and that launch 0 has survivors to compact."""
    from oracle import oracle
    from oracle.oracle import read_hrt
    assert len(CASES) == 17
    c = case_config("tie-r65537", tmp_path)
    meshes = read_hrt(c["scene_path"])
    assert sum(len(m["idx"]) for m in meshes) == TIE_TRI and meshes[0]["material_index"] != meshes[-1]["material_index"]
    assert (meshes[0]["vs"] == meshes[-1]["vs"]).all() and (meshes[0]["idx"] == meshes[-1]["idx"]).all()
    for scene, (n_tri, _) in SCENES.items():
        c = case_config(scene + "-r1000", tmp_path)
        assert sum(len(m["idx"]) for m in read_hrt(c["scene_path"])) == n_tri, scene
        live = [int(x) for x in oracle.compute_paths(*K.args(c))["extras"]["live"]]
        assert live[0] == 1000 and live[1] > 256, (scene, live)
    assert 1000 % 64 != 0 and -(-65537 // 256) == 257 and 65537 % 256 == 1 and 257 // 64 == 4
    assert 262145 == 256 * 1024 + 1 and -(-262145 // 1024) == 257 and 262145 % 1024 == 1
    assert (2 * 1000) // 64 > 1000 // 64 and 1000 % 64 != 0 and 65 > 64
    c = case_config("canyon-deep", tmp_path)
    assert (len(c["rx_pos"]), c["num_bounces"], c["num_paths"]) == (4, 3, 20000)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_launch0_is_bit_identical_to_the_oracle(name, tmp_path):
    p = subprocess.run([sys.executable, "-m", "tests.launch0_patch_child", name, str(tmp_path)], cwd=REPO,
                       capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
    print(p.stdout[-1500:])
    assert p.returncode == 0 and "LAUNCH0_OK " + name in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
