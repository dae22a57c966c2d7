"""Generate tests/golden/mcsweep_digests.json: per model of the marching-cubes sweep
(tests/mcsweep_util.py) its vertex and triangle counts and one SHA-256 over
parity_util.mesh_digests of the IEEE oracle's full output (per-MPU stats, positions, normals,
colours, MPU-local triangles).

The digests freeze the sweep's inputs and the oracle's bits on them: a change to the model
builder, to synth's boxes or to the oracle is noticed by tests/test_mcsweep.py without the
compiled reference at hand.

Usage: python tests/golden/make_mcsweep_digests.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import psoracle  # noqa: E402

import mcsweep_util as mu  # noqa: E402

psoracle.build()
out = {"generator": "oracle/psoracle.c (IEEE build), tests/mcsweep_util.models() at cell size 1",
       "entry": "[vertices, triangles, sha256 of json.dumps(parity_util.mesh_digests(...), sort_keys=True)]",
       "models": {}}
for name, _ in mu.models():
    out["models"][name] = mu.digest(mu.oracle_mesh(psoracle, name))
print(len(out["models"]), "models,", sum(v[0] for v in out["models"].values()), "vertices")
with open(os.path.join(HERE, "mcsweep_digests.json"), "w") as f:
    json.dump(out, f, indent=0)
    f.write("\n")
