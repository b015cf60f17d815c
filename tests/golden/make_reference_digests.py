#!/usr/bin/env python3
"""Record what the REAL reference computes for the parity cases that have no full golden arrays.

Runs oracle/_ref/libhrt_ref.so and oracle/_ref/sfs (built in place by `make -C oracle ref`, only
possible where the reference sources are present) and the reference's headers, and writes
tests/golden/reference_digests.json:

  <group>/<case>     SHA-256 and shape of every output array of compute_paths (both channel blocks,
                     RaysInfo snapshots, active masks, sentinels included) and of the normals it
                     leaves in the scene (tests/parity.py result_digests), for the cases of
                     test_oracle_vs_ref, test_edge_sizes, test_generated_scenes, test_in_plane_endpoints,
                     test_scaled_scenes and test_gpu_problem_tables
  importer/<scene>   SHA-256 of the .hrt the reference's importer CLI writes for its built-in scenes
  header_layout      sizeof / offsetof of every public struct and field of the reference's headers

The tests compare against these records, so they need neither the reference nor its build.
Nothing of the reference's code is stored: only inputs (named cases of the tests) and output data.

    python tests/golden/make_reference_digests.py <reference source directory>
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from hermespy_rt_amd import abi  # noqa: E402
from tests import configs as K  # noqa: E402
from tests.parity import result_digests  # noqa: E402

OUT = os.path.join(HERE, "reference_digests.json")

# struct -> fields, as named in both the reference's headers and include/hermespy_rt.h
LAYOUT = {
    "Vec3": ["x", "y", "z"],
    "Ray": ["o", "d"],
    "Mesh": ["num_vertices", "vs", "num_triangles", "is", "material_index", "velocity", "ns"],
    "Scene": ["num_meshes", "meshes"],
    "ChannelInfo": ["num_rays", "directions_rx", "directions_tx", "a_te_re", "a_te_im", "a_tm_re",
                    "a_tm_im", "tau", "freq_shift"],
    "RaysInfo": ["num_bounces", "num_rays", "rays", "rays_active"],
}


def layout_program(includes):
    """C source printing {"struct": [sizeof, {"field": offsetof}]} as JSON."""
    lines = ["#include <stddef.h>", "#include <stdio.h>"] + ['#include "%s"' % h for h in includes]
    lines.append("int main(void)\n{\n    printf(\"{\");")
    for i, (s, fields) in enumerate(LAYOUT.items()):
        offs = ", ".join('\\"%s\\": %%zu' % f for f in fields)
        args = ", ".join("offsetof(%s, %s)" % (s, f) for f in fields)
        lines.append('    printf("%s\\"%s\\": [%%zu, {%s}]", sizeof(%s), %s);'
                     % (", " if i else "", s, offs, s, args))
    lines.append('    printf("}\\n");\n    return 0;\n}')
    return "\n".join(lines) + "\n"


def header_layout(inc_dir, includes, tmp):
    src = os.path.join(tmp, "layout.c")
    exe = os.path.join(tmp, "layout")
    with open(src, "w") as f:
        f.write(layout_program(includes))
    subprocess.check_call(["gcc", "-O0", "-I", inc_dir, src, "-o", exe, "-lm"])
    return json.loads(subprocess.check_output([exe], text=True))


def cases(tmp):
    """group -> {case name: config}, exactly the cases the tests build."""
    from tests import (test_edge_sizes, test_generated_scenes, test_gpu_problem_tables,
                       test_oracle_vs_ref, test_scaled_scenes)
    groups = {"oracle_vs_ref": dict(test_oracle_vs_ref.CASES),
              "in_plane": dict(K.IN_PLANE),
              "problem_tables": dict(test_gpu_problem_tables.REF_CASES)}
    d = os.path.join(tmp, "edge")
    os.makedirs(d)
    groups["edge_sizes"] = {n: c for n, c in test_edge_sizes._cases(d).items() if n in test_edge_sizes.NAMES}
    d = os.path.join(tmp, "gen")
    os.makedirs(d)
    groups["generated_scenes"] = {n: test_generated_scenes.make(d, n) for n in test_generated_scenes.NAMES}
    d = os.path.join(tmp, "scaled")
    os.makedirs(d)
    groups["scaled_scenes"] = {n: test_scaled_scenes._case(d, n) for n in test_scaled_scenes.CASES}
    return groups


def main():
    from tests import refabi
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_inc = os.path.join(sys.argv[1], "inc")
    sfs = os.path.join(REPO, "oracle", "_ref", "sfs")
    if not refabi.available() or not os.path.exists(sfs) or not os.path.isdir(ref_inc):
        sys.exit("needs oracle/_ref/libhrt_ref.so and oracle/_ref/sfs (`make -C oracle ref`) and <reference>/inc")
    lib = refabi.load()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for group, cs in cases(tmp).items():
            out[group] = {}
            for name, c in cs.items():
                r = abi.run_compute_paths(lib, *K.args(c))
                out[group][name] = result_digests(r, np.concatenate(r["normals"]))
                print(group, name)
        out["importer"] = {}
        for name in ("box", "simple_reflector"):
            d = os.path.join(tmp, "sfs_" + name)
            os.makedirs(d)
            subprocess.check_call([sfs, "/x/%s.xml" % name], cwd=d, stdout=subprocess.DEVNULL)
            with open(os.path.join(d, "scene.hrt"), "rb") as f:
                out["importer"][name] = hashlib.sha256(f.read()).hexdigest()
        out["header_layout"] = header_layout(ref_inc, ["compute_paths.h", "scene.h"], tmp)
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
