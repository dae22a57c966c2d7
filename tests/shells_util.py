"""The inputs of the shells tests (tests/test_shells.py, tests/test_gpu_shells.py,
tests/golden/make_shell_counts.py): hand-made meshes whose answers are exact in binary, the
named weld inputs plus three built trees, and the counts both faces are compared by."""
import json
import os

import numpy as np

import weld_util
from parsip_amd import blobtree as bt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shell_counts.json")

TREE_CELLSIZE = 0.071
TREES = ("ring_union_point", "ring_point_apart", "cube_minus_point")
CASES = list(weld_util.CASES) + list(TREES)

COUNT_FIELDS = ("ctVertices", "ctTriangles", "ctEdges", "ctOpenEdges", "ctNonManifoldEdges", "ctFlippedEdges", "euler")


def make_tree(name):
    U, D = bt.BlobNodeType.OP_UNION, bt.BlobNodeType.OP_DIF
    ring = bt.Ring((.01, .02, .03), (0, 0, 1), 1.0)
    if name == "ring_union_point":      # touching: marching cubes leaves one non-manifold edge
        return bt.Op(U, ring, bt.Point((0, 0, 0)))
    if name == "ring_point_apart":      # a torus and a sphere
        return bt.Op(U, ring, bt.Point((3, 0, 0)))
    if name == "cube_minus_point":      # an inner cavity
        return bt.Op(D, bt.Cube((.01, .02, .03), 1.0), bt.Point((0, 0, 0)))
    raise KeyError(name)


def make_case(name):
    """(model, cellsize, (mpu_begin, mpu_end or None)) of a weld input or a built tree."""
    if name in TREES:
        code, model = bt.linearize_blobtree(bt.binarize(make_tree(name)), octrees="aabb")
        assert code == 0
        return model, TREE_CELLSIZE, (0, None)
    return weld_util.make_case(name)


def golden_counts():
    with open(GOLDEN) as f:
        return json.load(f)


def counts(sh):
    """A meshio.Shells as the golden file records it: integers, and the measures as floats."""
    info = sh.info
    out = {"shells": int(info["ctShells"]), "closed_shells": int(info["ctClosedShells"])}
    out.update({f: int(info[f]) for f in COUNT_FIELDS})
    out.update(area=float(info["area"]), volume=float(info["volume"]))
    out["per_shell"] = [dict({"firstVertex": int(s["firstVertex"])}, **{f: int(s[f]) for f in COUNT_FIELDS},
                             area=float(s["area"]), volume=float(s["volume"])) for s in sh.shells]
    return out


def integer_counts(c):
    """`counts` without the measures: what must match exactly on every machine."""
    out = {k: v for k, v in c.items() if k not in ("cellsize", "area", "volume", "per_shell")}
    out["per_shell"] = [{k: v for k, v in s.items() if k not in ("area", "volume")} for s in c["per_shell"]]
    return out


# ---- hand-made meshes ---------------------------------------------------------------------------

def cube(side=2.0, centre=(0.0, 0.0, 0.0)):
    """An axis-aligned cube, 8 vertices and 12 triangles wound outward."""
    h = side / 2.0
    pos = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float32) + np.float32(centre)
    # vertex id = 4 ix + 2 iy + iz; each face as two triangles, counter-clockwise seen from outside
    quads = [(0, 1, 3, 2), (4, 6, 7, 5),   # x = -h, x = +h
             (0, 4, 5, 1), (2, 3, 7, 6),   # y = -h, y = +h
             (0, 2, 6, 4), (1, 5, 7, 3)]   # z = -h, z = +h
    tris = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int64)
    return pos, tris


def two_cubes_interleaved():
    """Two cubes whose vertices alternate in the numbering: even ids cube A, odd ids cube B."""
    pa, ta = cube(2.0)
    pb, tb = cube(1.0, (4.0, 0.0, 0.0))
    pos = np.zeros((16, 3), np.float32)
    pos[0::2], pos[1::2] = pa, pb
    tris = np.concatenate([np.stack([2 * ta[i], 2 * tb[i] + 1]) for i in range(12)])  # triangles alternate too
    return pos, tris


def fan():
    """Three triangles on the edge 0-1."""
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    return pos, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int64)
