"""Deterministic trees and lattices at the compat mode's limits (tests/test_gpu_gui_limits.py):
tree sizes around the 64- and 128-node live masks, operator nesting at PSGUI_MAX_DEPTH,
bare primitives (no operator), n-ary folds up to the converter's 1,024 kids, and lattices
around the offsets scan's 1,024-MPU blocks.  No RNG: every position, kind and parameter is a
function of the node's index."""
import math

import numpy as np

from gui_util import PRIM_KINDS
from parsip_amd import blobtree as bt
from parsip_amd import gui

B = bt.BlobNodeType
MAX_DEPTH = 32  # PSGUI_MAX_DEPTH (include/parsip_gpu_gui.h)
FOLD_OPS = (B.OP_BLEND, B.OP_UNION, B.OP_RICCIBLEND)
CHAIN_OPS = (B.OP_UNION, B.OP_BLEND, B.OP_RICCIBLEND, B.OP_DIF, B.OP_SMOOTHDIF, B.OP_INTERSECT)
AXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))


def _frac(i, k):
    """A fixed pseudo-jitter in [0, 1): the fractional part of i * k * the golden ratio."""
    return (i * k * 0.6180339887498949) % 1.0


def _colour(i):
    return bt.Material(diffused=(0.1 + 0.8 * _frac(i, 1), 0.1 + 0.8 * _frac(i, 2), 0.1 + 0.8 * _frac(i, 3), 1.0))


def _small_affine(i):
    """A mild transform of its own: a rotation about an axis, an anisotropic scale, a shift."""
    ang = 0.2 + 0.5 * _frac(i, 5)
    ax = AXES[i % 3]
    q = tuple(math.sin(ang / 2) * a for a in ax) + (math.cos(ang / 2),)
    return bt.Affine((1.0 + 0.2 * _frac(i, 7), 1.0, 1.0 - 0.15 * _frac(i, 11)), q,
                     (0.1 * _frac(i, 13), -0.1 * _frac(i, 17), 0.05))


def grid_prim(i, n, spacing):
    """Primitive i of n on a cubic grid centred on the origin: kinds of PRIM_KINDS cycled,
    every seventh under a transform of its own."""
    side = max(1, math.ceil(round(n ** (1.0 / 3.0), 9)))
    ix, iy, iz = i % side, (i // side) % side, i // (side * side)
    h = 0.5 * (side - 1)
    c = (spacing * (ix - h) + 0.1 * (_frac(i, 19) - 0.5), spacing * (iy - h) + 0.1 * (_frac(i, 23) - 0.5),
         spacing * (iz - h) + 0.1 * (_frac(i, 29) - 0.5))
    kw = {"material": _colour(i)}
    if i % 7 == 3:
        kw["transform"] = _small_affine(i)
    k = PRIM_KINDS[i % len(PRIM_KINDS)]
    d = AXES[(i // len(PRIM_KINDS)) % 3]
    e = tuple(c[a] + 0.4 * d[a] for a in range(3))
    if k == "point":
        return bt.Point(c, **kw)
    if k == "line":
        return bt.Line(c, e, **kw)
    if k == "cylinder":
        return bt.Cylinder(c, d, 0.1 + 0.1 * _frac(i, 3), 0.3, **kw)
    if k == "disc":
        return bt.Disc(c, d, 0.25, **kw)
    if k == "ring":
        return bt.Ring(c, d, 0.3, **kw)
    if k == "cube":
        return bt.Cube(c, 0.12 + 0.1 * _frac(i, 5), **kw)
    if k == "triangle":
        f = AXES[(i // len(PRIM_KINDS) + 1) % 3]
        return bt.Triangle(c, e, tuple(c[a] + 0.35 * f[a] for a in range(3)), **kw)
    if k == "quadric":
        return gui.QuadricPoint(c, 0.9, 1.2, **kw)
    return bt.Null(**kw)


def balanced(nodes):
    """A balanced tree over `nodes`: BLEND / UNION / RICCIBLEND (n = 2 and 3.5 in turn) with
    2, 3, 4 kids in turn, every fifth operator under a transform of its own."""
    level, c = list(nodes), 0
    while len(level) > 1:
        nxt, i = [], 0
        while i < len(level):
            k = 2 + c % 3
            grp = level[i:i + k]
            i += k
            if len(grp) == 1:  # a lone rest goes up as it is
                nxt.append(grp[0])
                continue
            kind = FOLD_OPS[(c + c // 3) % 3]
            op = bt.Op(kind, *grp, **({"n": (2.0, 3.5)[c % 2]} if kind == B.OP_RICCIBLEND else {}))
            if c % 5 == 4:
                op.transform = _small_affine(100 + c)
            nxt.append(op)
            c += 1
        level = nxt
    return level[0]


def prim_count_tree(n_prims, spacing=0.6):
    """Section 1: n_prims grid primitives under a balanced tree."""
    root = balanced([grid_prim(i, n_prims, spacing) for i in range(n_prims)])
    return root if root.is_operator() else bt.Op(B.OP_UNION, root)


def _count_ops(n):
    return 1 + sum(_count_ops(c) for c in n.children) if n.is_operator() else 0


def op_count_tree(n_ops, n_prims=40, spacing=0.6):
    """Section 1: exactly n_ops operators over n_prims (<= 64) primitives.  The balanced tree's
    operators, and unary operators around the primitives to make up the count: a UNION of one
    kid, and around the last eighth of the primitives a gentle one-kid shear warp (the
    primitives below a warp have no culling box)."""
    leaves = [grid_prim(i, n_prims, spacing) for i in range(n_prims)]
    need = n_ops - _count_ops(balanced([bt.Null() for _ in range(n_prims)]))
    assert need >= 0, (n_ops, n_prims)
    for w in range(need):
        j = w % n_prims
        if j >= n_prims - n_prims // 8 and w < n_prims:
            leaves[j] = bt.Op(B.OP_WARPSHEAR, leaves[j], resX=0.15, resY=float(j % 3), resZ=float((j + 1) % 3))
        else:
            leaves[j] = bt.Op(B.OP_UNION, leaves[j])
    return balanced(leaves)


def _chain_affine(i):
    """The chain's own transforms are slight: thirty levels of them leave the ring a ring."""
    ang = 0.04 + 0.04 * _frac(i, 5)
    q = tuple(math.sin(ang / 2) * a for a in AXES[i % 3]) + (math.cos(ang / 2),)
    return bt.Affine((1.0 + 0.03 * _frac(i, 7), 1.0, 1.0 - 0.03 * _frac(i, 11)), q, (0.02, -0.01, 0.015))


def _ring_prim(i):
    """A level's primitive: on a ring of radius 1.5 about the core, overlapping its neighbours
    (0.33 apart) and exactly +0 in the core."""
    a = 0.22 * i
    c = (1.5 * math.cos(a), 1.5 * math.sin(a), 0.1 * (_frac(i, 3) - 0.5))
    if i % 4 == 1:
        return bt.Cube(c, 0.15, material=_colour(i))
    if i % 4 == 3:
        return bt.Line(c, (c[0], c[1], c[2] + 0.3), material=_colour(i))
    return bt.Point(c, material=_colour(i))


def depth_chain(depth, first=0):
    """Section 2: `depth` nested operators, kinds of CHAIN_OPS cycled from the root (a UNION),
    each with one primitive beside the nested operator; every fifth under a transform.

    The innermost operator blends two POINTs in the core (near the origin); its value reaches
    the root there, so a frame lost at the bottom of the stack shows: every level's primitive
    is exactly +0 in the core (UNION, BLEND, RICCIBLEND pass the nested value on; DIF and
    SMOOTHDIF do with the nested kid first, as they have it here), and INTERSECT's is a CUBE
    that is 1 over the whole scene.  The symmetric operators take the nested kid first and
    last in turn."""
    node = None
    for lvl in range(depth, 0, -1):  # the innermost first
        kind = CHAIN_OPS[(lvl - 1) % len(CHAIN_OPS)]
        prm = {"n": 2.0} if kind == B.OP_RICCIBLEND else {}
        if kind == B.OP_INTERSECT:
            p = bt.Cube((0.0, 0.0, 0.0), 2.5, material=_colour(first + lvl))
        else:
            p = _ring_prim(first + lvl)
        if node is None:
            kids = [bt.Point((-0.12, 0.03, 0.0), material=_colour(first + 90)),
                    bt.Point((0.15, -0.02, 0.05), material=_colour(first + 91))]
            kind, prm = B.OP_BLEND, {}
        elif kind in (B.OP_DIF, B.OP_SMOOTHDIF) or lvl % 2 == 0:
            kids = [node, p]
        else:
            kids = [p, node]
        node = bt.Op(kind, *kids, **prm)
        if lvl % 5 == 0:
            node.transform = _chain_affine(lvl)
    return node


def instance_chain(d, h):
    """Section 2, the extended walk: the root UNION holds an origin subtree of height h (a
    depth chain) and a chain of UNION / BLEND operators whose operator at depth d holds an
    Instance of that origin: the walk's stack is d + h frames deep there."""
    origin = depth_chain(h, first=40)
    inst = bt.Instance(origin, transform=bt.Affine((1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 1.0), (0.9, 0.2, 0.0)),
                       material=_colour(77))
    node = None
    for lvl in range(d, 1, -1):
        kind = (B.OP_UNION, B.OP_BLEND)[lvl % 2]
        p = bt.Point((0.9 + 0.3 * math.cos(lvl), 0.2 + 0.3 * math.sin(lvl), 0.02 * lvl), material=_colour(lvl))
        node = bt.Op(kind, inst, p) if node is None else bt.Op(kind, *([node, p] if lvl % 2 else [p, node]))
    return bt.Op(B.OP_UNION, origin, node)


def bare_prim(name):
    """Section 3: a primitive as the whole tree."""
    if name == "point":
        return bt.Point((0.1, -0.2, 0.05), material=_colour(1))
    if name == "cube":
        return bt.Cube((0.0, 0.1, -0.1), 0.3, material=_colour(2))
    assert name == "cylinder"
    return bt.Cylinder((0.1, 0.0, 0.0), (0.0, 0.0, 1.0), 0.2, 0.5, material=_colour(3),
                       transform=bt.Affine((1.2, 0.9, 1.0), (0.0, 0.25881905, 0.0, 0.9659258), (0.2, -0.1, 0.1)))


def nary_points(n, extent):
    """n POINT centres on a jittered grid in [-extent, extent]^3; the first sits in the lower
    corner and the last in the upper one, so the tree's octree is [-extent - 0.5, extent + 0.5]^3."""
    side = math.ceil(round(n ** (1.0 / 3.0), 9))
    step = 2.0 * extent / (side - 1)
    cells = [(i % side, (i // side) % side, i // (side * side)) for i in range(side ** 3)]
    # n of the side^3 grid points, spread evenly, the two corners among them
    pick = [cells[round(j * (side ** 3 - 1) / (n - 1))] for j in range(n)]
    out = []
    for j, (ix, iy, iz) in enumerate(pick):
        g = [-extent + step * v for v in (ix, iy, iz)]
        if 0 < j < n - 1:  # jitter toward the centre: nothing leaves the cube
            for a in range(3):
                g[a] -= math.copysign(0.3 * step * _frac(j, 31 + a), g[a]) if g[a] != 0.0 else 0.0
        out.append(tuple(g))
    return out


def nary_tree(kind, n_kids, ricci_n=None, extent=2.0, first=0):
    """Section 4: one operator over n_kids POINTs; kid 0 is point `first` of the grid."""
    pts = nary_points(n_kids, extent)
    pts = pts[first:] + pts[:first]
    kids = [bt.Point(c, material=_colour(j)) for j, c in enumerate(pts)]
    return bt.Op(kind, *kids, **({"n": ricci_n} if kind == B.OP_RICCIBLEND else {}))


def tree_shape(tree):
    """(primitives, operators, largest kid count, nesting depth) of a compact tree."""
    if tree.ct_ops == 0:
        return tree.ct_prims, 0, 0, 0

    def depth(op):
        o = tree.ops[op]
        ks = tree.kids[int(o["kidStart"]):int(o["kidStart"]) + int(o["ctKids"])]
        return 1 + max([depth(int(k) & 0xFFFF) for k in ks if int(k) >> 16], default=0)

    return tree.ct_prims, tree.ct_ops, int(tree.ops["ctKids"].max()), depth(0)


def convert(root):
    code, tree = gui.compact_blobtree(root)
    assert code == 0, code
    return tree


# ---- lattices ---------------------------------------------------------------
LATTICE_CS = 0.125             # exact in binary: an MPU is 0.875 wide, every corner below exact
MPU_SIDE = 7 * LATTICE_CS
LATTICE_LO = (-0.4375, -0.4375, -0.4375)
LATTICE_DIMS = {1: (1, 1, 1), 1023: (1, 1, 1023), 1024: (1024, 1, 1), 1025: (1, 1025, 1), 2048: (2, 32, 32),
                2049: (683, 1, 3), 1092727: (103, 103, 103)}


def lattice_octree(dims):
    lo = np.array(LATTICE_LO, np.float32)
    hi = (lo.astype(np.float64) + MPU_SIDE * np.array(dims, np.float64)).astype(np.float32)
    return lo, hi


def lattice_dims(lo, hi, cs):
    """CParsipOptimized::setup's lattice: ceil(side / cellsize) cells, MPUs of 7 cells."""
    cells = np.ceil((np.asarray(hi, np.float32) - np.asarray(lo, np.float32)) / np.float32(cs)).astype(np.int64)
    return tuple(int(c) // 7 + (1 if int(c) % 7 else 0) for c in cells)


def mpu_centre(dims, m):
    k, j, i = m % dims[2], (m // dims[2]) % dims[1], m // (dims[2] * dims[1])
    return tuple(LATTICE_LO[a] + MPU_SIDE * (v + 0.5) for a, v in enumerate((i, j, k)))


def one_point_tree(dims):
    """A POINT under a UNION in the middle MPU of the lattice."""
    n = dims[0] * dims[1] * dims[2]
    return bt.Op(B.OP_UNION, bt.Point(mpu_centre(dims, n // 2), material=_colour(5)))


def three_point_tree(dims):
    """POINTs in the first, a middle and the very last MPU: the scan's offsets are nonzero
    from the first MPU on and change in the last."""
    n = dims[0] * dims[1] * dims[2]
    return bt.Op(B.OP_UNION, *[bt.Point(mpu_centre(dims, m), material=_colour(6 + q))
                               for q, m in enumerate((0, n // 2, n - 1))])
