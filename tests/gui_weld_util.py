"""Shared helpers of the compat-mode weld tests (test_gui_weld.py on the CPU oracle,
test_gpu_gui_weld.py on the device): the six inputs of tests/golden/gui_weld_counts.json, their
lattices, and the figures the golden file records."""
import json
import os
from functools import lru_cache

import numpy as np
from gui_util import random_ext_tree, random_tree

from parsip_amd import blobtree as bt
from parsip_amd import gui, meshio

B = bt.BlobNodeType
ISO = 0.5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gui_weld_counts.json")


def _sphere():
    return bt.Op(B.OP_UNION, bt.Point((0.1, 0.05, -0.02)))


# name -> (root builder, cellsize): lattices 1x1x1 (36 vertices: below one wave, no seam, an
# empty table), 2x2x2, 3x3x3, 4x2x2, 6x4x6 and 4x2x3; V mod 4 = 0, 2, 0, 3, 1, 1
CASES = {
    "sphere_cs0.3": (_sphere, 0.3),
    "sphere_cs0.13": (_sphere, 0.13),
    "sphere_cs0.071": (_sphere, 0.071),
    "random3_cs0.13": (lambda: random_tree(3, 6, warps=False), 0.13),
    "random5_cs0.1": (lambda: random_tree(5, 8), 0.1),
    "ext1_cs0.15": (lambda: random_ext_tree(1), 0.15),
}


@lru_cache(maxsize=None)
def make_tree(name):
    """(CompactTree, cellsize) of a case; the lattice is over the tree's root octree at ISO."""
    build, cs = CASES[name]
    code, tree = gui.compact_blobtree(build())
    assert code >= 0, (name, code)
    return tree, cs


def lattice_dims(tree, cs):
    """CParsipOptimized::setup's MPU lattice (psgpu_gui_polygonize: ceil(side / cs) cells in
    float32, MPUs of 7 cells)."""
    lo, hi = (np.asarray(v, np.float32)[:3] for v in tree.root_octree)
    cells = np.ceil(((hi - lo) / np.float32(cs)).astype(np.float64)).astype(np.int64)
    return tuple(int(c) // 7 + (1 if int(c) % 7 else 0) for c in cells)


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def degenerate_count(tris) -> int:
    t = np.asarray(tris).reshape(-1, 3)
    return int(((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])).sum())


def mpu_of_vertex(mpu_v) -> np.ndarray:
    mpu_v = np.asarray(mpu_v, np.int64)
    return np.repeat(np.arange(len(mpu_v) - 1, dtype=np.int64), np.diff(mpu_v))


def weld_figures(mesh, edges, cs) -> dict:
    """What the golden file records of one input: `mesh` a GuiMesh (or the oracle's result),
    `edges` its vertices' lattice edges."""
    tm = meshio.TriMesh(mesh.pos, mesh.tris.astype(np.int64), mesh.nrm, mesh.col)
    w, vmap = meshio.weld_by_edges(tm, edges)
    sh = meshio.shells(w.pos, w.tris)
    copies = np.bincount(vmap, minlength=w.n_vertices)
    first = np.full(w.n_vertices, len(vmap), np.int64)
    np.minimum.at(first, vmap, np.arange(len(vmap)))
    rep = first[vmap]                                   # every input vertex's representative
    d = np.linalg.norm(mesh.pos.astype(np.float64) - mesh.pos[rep].astype(np.float64), axis=1)
    pb = mesh.pos.view(np.uint32).reshape(-1, 3)
    nd = np.abs(mesh.nrm.astype(np.float64) - mesh.nrm[rep].astype(np.float64)).max(axis=1)
    wb = bit_weld_unfiltered(tm)
    return {
        "vertices": int(len(mesh.pos)), "triangles": int(len(mesh.tris)),
        "edge_weld": {"vertices": w.n_vertices, "open_edges": meshio.open_edge_count(w.tris),
                      "degenerate": degenerate_count(w.tris), "shells": int(sh.info["ctShells"]),
                      "euler": [int(e) for e in sh.shells["euler"]]},
        "bit_weld": {"vertices": wb[0], "degenerate": wb[1]},
        "vertices_with_copy": int((copies[vmap] > 1).sum()),
        "max_copies": int(copies.max()) if len(copies) else 0,
        "copies_bits_differ": int((pb != pb[rep]).any(axis=1).sum()),
        "max_copy_distance_cs": float(d.max() / cs) if len(d) else 0.0,
        "max_copy_normal_diff": float(nd.max()) if len(nd) else 0.0,
    }


def bit_weld_unfiltered(tm):
    """(welded vertices, degenerate triangles) of the position-bit weld: `meshio.weld` drops the
    triangles that collapse, so they are its input's minus its output's."""
    wb = meshio.weld(tm)
    return wb.n_vertices, tm.n_triangles - wb.n_triangles
