"""Regenerate tests/golden/weld_counts.json: for each named input, the oracle mesh's vertex and
triangle counts, and vertices / open edges (edges used by exactly one triangle) after
`meshio.weld` (position bits) and after `meshio.weld_lattice` (lattice-edge identity).

    python3 tests/golden/make_weld_counts.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

sys.path.insert(0, os.path.join(ROOT, "tests"))

import psoracle  # noqa: E402
from weld_util import CASES, make_case  # noqa: E402

from parsip_amd import meshio  # noqa: E402


def main():
    psoracle.build()
    out = {}
    for name in CASES:
        model, cs, (b, e) = make_case(name)
        e = 0xFFFFFFFF if e is None else e
        om = psoracle.polygonize(model, cs, b, e, threads=8)
        m = meshio.TriMesh(om.pos, om.global_tris(), om.nrm, om.col)
        wb = meshio.weld(m)
        wl, _ = meshio.weld_lattice(m, om.vertex_offsets, cs, *model.bbox, mpu_begin=b)
        out[name] = {"cellsize": cs, "mpus": len(om.stats), "vertices": m.n_vertices, "triangles": m.n_triangles,
                     "bit_weld": {"vertices": wb.n_vertices, "open_edges": meshio.open_edge_count(wb.tris)},
                     "lattice_weld": {"vertices": wl.n_vertices, "triangles": wl.n_triangles,
                                      "open_edges": meshio.open_edge_count(wl.tris)}}
    with open(os.path.join(HERE, "weld_counts.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
