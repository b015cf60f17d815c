""".hrt scene I/O of the product library (host-only entry points scene_load / scene_save,
drop-ins for src/scene.c:7-83): parsed contents equal the oracle's independent reader,
save(load(f)) is byte-identical to f for all bundled scenes, error status is exit(8)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi
from oracle import oracle

from . import configs as K

SCENES = ["box.hrt", "simple_reflector.hrt", "2cars.hrt", "simple_street_canyon_with_cars.hrt"]
EXPECT = {"box.hrt": (1, 12), "simple_reflector.hrt": (1, 2), "2cars.hrt": (3, 26),
          "simple_street_canyon_with_cars.hrt": (15, 234)}   # meshes, triangles


@pytest.mark.parametrize("name", SCENES)
def test_load_matches_independent_reader(product_lib, name):
    path = os.path.join(K.SC, name)
    sc = product_lib.scene_load(path.encode())
    try:
        got = abi.scene_to_numpy(sc)
    finally:
        abi.free_scene(sc)
    want = oracle.read_hrt(path)
    assert (len(got), sum(len(m["idx"]) for m in got)) == EXPECT[name]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(g["vs"].view(np.uint32), w["vs"].view(np.uint32))
        assert np.array_equal(g["idx"], w["idx"])
        assert g["material_index"] == w["material_index"]
        assert np.array_equal(g["velocity"], w["velocity"])
        assert g["ns"] is None   # the loader does not compute normals (inc/scene.h:23-26)


@pytest.mark.parametrize("name", SCENES)
def test_save_roundtrip_byte_identical(product_lib, name, tmp_path):
    path = os.path.join(K.SC, name)
    sc = product_lib.scene_load(path.encode())
    out = tmp_path / "out.hrt"
    try:
        product_lib.scene_save(C.byref(sc), str(out).encode())
    finally:
        abi.free_scene(sc)
    assert out.read_bytes() == open(path, "rb").read()


def test_importer_goldens_match_bundled_scenes(product_lib, tmp_path):
    """The reference importer's two hard-coded scenes (their SHA-256 recorded by
    tests/golden/make_reference_digests.py) reproduce box.hrt / simple_reflector.hrt byte for byte
    (SURVEY.md section 10); our scene_save re-emits the same bytes."""
    with open(os.path.join(K.REPO, "tests", "golden", "reference_digests.json")) as f:
        want = json.load(f)["importer"]
    for name in ("box", "simple_reflector"):
        ref_bytes = open(os.path.join(K.SC, name + ".hrt"), "rb").read()
        assert hashlib.sha256(ref_bytes).hexdigest() == want[name]
        (tmp_path / "scene.hrt").write_bytes(ref_bytes)
        sc = product_lib.scene_load(str(tmp_path / "scene.hrt").encode())
        product_lib.scene_save(C.byref(sc), str(tmp_path / "ours.hrt").encode())
        abi.free_scene(sc)
        assert (tmp_path / "ours.hrt").read_bytes() == ref_bytes


@pytest.mark.parametrize("content", [None, b"", b"HR", b"XYZ\x01\x00\x00\x00", b"HRT\x00\x00\x00\x00",
                                     b"HRT\xe9\x03\x00\x00", b"HRT\x01\x00\x00\x00\x05\x00\x00\x00"])
def test_bad_files_exit_8(content, tmp_path):
    """src/scene.c:36-76: any open/parse failure ends the process with status 8."""
    p = tmp_path / "bad.hrt"
    if content is not None:
        p.write_bytes(content)
    code = ("import sys; sys.path.insert(0, %r)\nfrom hermespy_rt_amd import lib\n"
            "lib.load().scene_load(%r)\n" % (K.REPO, str(p).encode()))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True)
    assert r.returncode == 8, (content, r.returncode, r.stderr[-300:])
