"""Regenerate tests/golden/gui_weld_counts.json: for each input of tests/gui_weld_util.py, the CPU
oracle's compat mesh (oracle/psgui.py) welded by lattice-edge identity (`gui.lattice_edges` with
the oracle's field, `meshio.weld_by_edges`) and by position bits (`meshio.weld`): vertices, open
edges, degenerate triangles, shells and their Euler characteristics; how many input vertices
have a copy, the most copies of one welded vertex, how many copies differ in position bits from
their representative, and the largest distance between a copy and its representative in cell
sizes.  `copy_distance_bound_cs`, the geometric bound the tests use, is the largest of those
distances times 8: the margin is for other trees' conditioning, it is no property of a device.

    python3 tests/golden/make_gui_weld_counts.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import psgui  # noqa: E402
from gui_weld_util import CASES, ISO, lattice_dims, make_tree, weld_figures  # noqa: E402

from parsip_amd import gui  # noqa: E402


def main():
    out = {"cases": {}}
    for name in CASES:
        tree, cs = make_tree(name)
        om = psgui.polygonize(tree, *tree.root_octree, cs, ISO, threads=8)
        dims = lattice_dims(tree, cs)
        assert dims == tuple(om.info.dims), (dims, tuple(om.info.dims))
        edges = gui.lattice_edges(om, dims, tree.root_octree[0], cs, ISO, lambda p: psgui.field_values(tree, p)[0])
        out["cases"][name] = dict({"cellsize": cs, "dims": list(dims)}, **weld_figures(om, edges, cs))
    out["copy_distance_bound_cs"] = 8.0 * max(c["max_copy_distance_cs"] for c in out["cases"].values())
    with open(os.path.join(HERE, "gui_weld_counts.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
