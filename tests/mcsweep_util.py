"""The marching-cubes sweep: every cell configuration in every cell position (tests/test_mcsweep.py
on the CPU oracle, tests/test_gpu_mcsweep.py on the device, tests/golden/make_mcsweep_digests.py;
DESIGN.md §2 "The marching-cubes sweep").

At cell size 1 over the box [0, 14]^3 (a 2x2x2 MPU lattice) the lattice corners are the integer
points.  A POINT on a corner has field exactly 1 there and exactly 0 at every other corner (field
radius 1), so under UNION the inside corners are exactly the points: the *outside* background.
DIF(UNION(cube over the box, far point), UNION(points)) is its complement, every corner inside
but the points: the *inside* background.  A configuration (bit c = x*4 + y*2 + z set: corner c of
the cell is inside, psoracle.c) of at most 4 inside corners is written with that many points on
the outside background, one of more with at most 3 points on the inside background.

A cell's position class has, per axis, 0: local i == 0 (the low cells of the box), 1: 0 < i < 6,
2: i == 6 (the far face is an MPU seam or a box face); 27 classes, whose ownership projection
(i == 0, j == 0, k == 0) selects CubeTablesDev::own.  The *sites* are the cells at global
coordinates 0, 2, 4, 6, 9, 11, 13 per axis (local 0, 2, 4, 6 of the first MPU, 2, 4, 6 of the
second): no two share a corner, so every site holds exactly the configuration written into it;
the cells between take what results.

Model m of a background that has N configurations writes, for each of the 27 classes, the
configuration of index (m + shift of the class) mod N into one site of the class (which of the
class's sites turns with m and the class, per axis, which spreads a model's sites over the eight
MPUs), so the N models of a background put every configuration into every class once: 162 + 92 =
254 models.  The configurations are ordered by their number of
points and the shifts are spread evenly over N, so every model draws from every count alike and
needs about the mean number of points (85.3 of the outside background, 68.1 of the inside one).
Each background's models are padded with POINTs far outside the box to one primitive count, so
that each has one tree structure (one compile of the structure-specialised kernels).  The outside
background carries two anchor POINTs off the lattice, beside the corners (7, 7, 7), which every
MPU has, and (14, 14, 14): field 0.0156 there, below 0.125 on every lattice edge, so S1 passes
the MPUs and no crossing moves.  No RNG anywhere."""
import os

import numpy as np

from parsip_amd import soa, synth
from parsip_amd.soa import NodeType

CS = 1.0
DIMS = (2, 2, 2)
CELLS = {0: (0,), 1: (2, 4, 9, 11), 2: (6, 13)}     # per axis: position class -> global cell coordinates of the sites
CLASSES = [(a, b, c) for a in range(3) for b in range(3) for c in range(3)]
FAR = (-40.0, -40.0, -40.0)
ANCHORS = ((6.5, 6.5, 6.5), (13.5, 13.5, 13.5))
CUBE = ((7.0, 7.0, 7.0), 8.0)                        # centre, half side: field 1 over the whole box
BACKGROUNDS = ("out", "in")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mcsweep_digests.json")

_MODELS = []
_ORACLE = {}
_N_POINTS = {}


def popcount(c):
    return bin(c).count("1")


def configs(background):
    """The configurations a background writes, by their number of points, then by value."""
    if background == "out":
        return sorted((c for c in range(1, 255) if popcount(c) <= 4), key=lambda c: (popcount(c), c))
    return sorted((c for c in range(1, 255) if popcount(c) > 4), key=lambda c: (-popcount(c), c))


def sites(background, m):
    """[(cell (gx, gy, gz), configuration)] of model m of a background: one site per class."""
    cfgs = configs(background)
    n = len(cfgs)
    out = []
    for q, cl in enumerate(CLASSES):
        cell = tuple(CELLS[c][(m + (q >> a)) % len(CELLS[c])] for a, c in enumerate(cl))
        out.append((cell, cfgs[(m + (q * n) // len(CLASSES)) % n]))
    return out


def flipped_corners(background, m):
    """The lattice corners that carry a POINT in model m: the inside corners of its sites'
    configurations on the outside background, the outside ones on the inside background."""
    want = 1 if background == "out" else 0
    pts = []
    for (gx, gy, gz), cfg in sites(background, m):
        for c in range(8):
            if (cfg >> c) & 1 == want:
                pts.append((gx + (c >> 2 & 1), gy + (c >> 1 & 1), gz + (c & 1)))
    assert len(set(pts)) == len(pts)  # no two sites share a corner
    return pts


def n_points(background):
    """The POINT count every model of a background is padded to: the most any of them needs."""
    if background not in _N_POINTS:
        _N_POINTS[background] = max(len(flipped_corners(background, m)) for m in range(len(configs(background))))
    return _N_POINTS[background]


def union_tree(O, counter, a, b):
    """A balanced UNION tree over primitives [a, b), op ids in pre-order from counter[0] on;
    returns (is_op, id) of its root (a lone primitive is its own root)."""
    if b - a == 1:
        return 0, a
    op = counter[0]
    counter[0] += 1
    mid = (a + b) // 2
    lk, lid = union_tree(O, counter, a, mid)
    rk, rid = union_tree(O, counter, mid, b)
    set_op(O, op, NodeType.UNION, (lk, lid), (rk, rid))
    return 1, op


def set_op(O, op, op_type, left, right):
    O["opType"][0, op] = op_type
    O["opLeftChild"][0, op], O["opRightChild"][0, op] = left[1], right[1]
    O["opChildKind"][0, op] = left[0] * 2 + right[0]


def build(background, m):
    """Model m of a background (see the module's text)."""
    pts = flipped_corners(background, m)
    pad = n_points(background) - len(pts)
    model = soa.Model.empty("mc_%s%03d" % (background, m))
    O = model.ops
    head = [(NodeType.POINT, a) for a in ANCHORS] if background == "out" else \
        [(NodeType.CUBE, CUBE[0]), (NodeType.POINT, FAR)]
    prims = head + [(NodeType.POINT, p) for p in pts] + [(NodeType.POINT, FAR)] * pad
    assert len(prims) <= soa.MAX_TREE_NODES
    for i, (t, at) in enumerate(prims):
        synth.set_prim(model, i, t, np.asarray(at, np.float32) * np.float32(CS))
        if t == NodeType.CUBE:
            model.prims["resX"][0, i] = CUBE[1] * CS
    model.prims["ctPrims"][0] = len(prims)
    counter = [0]
    if background == "out":
        union_tree(O, counter, 0, len(prims))
    else:  # the root's children are both operators, so the tree split takes the tree
        counter[0] = 1
        left = union_tree(O, counter, 0, 2)
        right = union_tree(O, counter, 2, len(prims))
        assert left[0] == 1 and right[0] == 1
        set_op(O, 0, NodeType.DIF, left, right)
    O["ctOps"][0] = counter[0]
    synth.prepare_boxes(model)
    model.prims["bboxLo"][0] = (0.0, 0.0, 0.0)
    model.prims["bboxHi"][0] = tuple(np.float32(7 * d) * np.float32(CS) for d in DIMS)
    assert soa.mpu_dims(CS, *model.bbox) == DIMS
    return model


def models():
    """(name, model) of the sweep's 254 models, the outside background first (built once per
    process, shared, never modified)."""
    if not _MODELS:
        for bg in BACKGROUNDS:
            for m in range(len(configs(bg))):
                model = build(bg, m)
                _MODELS.append((model.name, model))
    return iter(_MODELS)


def names():
    return [n for n, _ in models()]


def model_of(name):
    return dict(models())[name]


def structure(model):
    """What the structure-specialised kernels are compiled from: the tree and the node types."""
    P, O = model.prims, model.ops
    n, k = model.ct_prims, model.ct_ops
    return (n, k, P["skeletType"][0, :n].tobytes(), P["idxMatrix"][0, :n].tobytes()) + \
        tuple(O[f][0, :k].tobytes() for f in ("opType", "opLeftChild", "opRightChild", "opChildKind"))


def oracle_mesh(oracle, name, sse_approx=False):
    """The oracle's mesh of a model (the IEEE build's unless sse_approx), computed once per process."""
    key = (name, sse_approx)
    if key not in _ORACLE:
        om = oracle.polygonize(model_of(name), CS, threads=1, sse_approx=sse_approx)
        for a in (om.stats, om.pos, om.nrm, om.col, om.tris):
            a.setflags(write=False)
        _ORACLE[key] = om
    return _ORACLE[key]


def digest(om):
    """[vertices, triangles, one SHA-256 over parity_util.mesh_digests] of an oracle mesh: an
    entry of tests/golden/mcsweep_digests.json."""
    import hashlib
    import json

    from parity_util import mesh_digests

    d = mesh_digests(om.stats[:, :4], om.pos, om.nrm, om.col, om.tris)
    return [d["vertices"], d["triangles"], hashlib.sha256(json.dumps(d, sort_keys=True).encode()).hexdigest()]


def mpu_configs(oracle, model):
    """(ctMPUs, 7, 7, 7) cell configurations of every MPU from oracle.field_value at its 8^3
    corners (z fastest, so that groups of 4 points are the reference's S2 quads)."""
    org = soa.mpu_origins(CS, *model.bbox)
    steps = np.float32(CS) * np.arange(8, dtype=np.float32)
    g = np.stack(np.meshgrid(steps, steps, steps, indexing="ij"), axis=-1).reshape(-1, 3)   # z fastest
    p = (org[:, None, :] + g[None, :, :]).astype(np.float32).reshape(-1, 3)
    f = oracle.field_value(model, p[:, 0], p[:, 1], p[:, 2]).reshape(len(org), 8, 8, 8)
    ins = (f >= np.float32(0.5)).astype(np.int64)
    cfg = np.zeros((len(org), 7, 7, 7), np.int64)
    for c in range(8):
        x, y, z = c >> 2 & 1, c >> 1 & 1, c & 1
        cfg |= ins[:, x:x + 7, y:y + 7, z:z + 7] << c
    return cfg


# the position class of every cell of an MPU: (7, 7, 7) of class ids 9 a + 3 b + c
_AXIS_CLASS = np.array([0, 1, 1, 1, 1, 1, 2])
CELL_CLASS = 9 * _AXIS_CLASS[:, None, None] + 3 * _AXIS_CLASS[None, :, None] + _AXIS_CLASS[None, None, :]


def coverage(oracle, model):
    """(256, 27) histogram of (configuration, position class) over the cells of the MPUs the
    oracle polygonized (passed S1 and has triangles).  Here the class is the cell's own, in its
    MPU: an i == 0 cell of the second MPU counts for class 0 too."""
    om = oracle_mesh(oracle, model.name) if model.name in names() else oracle.polygonize(model, CS)
    done = (om.stats[:, 0] != 0) & (om.stats[:, 3] != 0)
    cfg = mpu_configs(oracle, model)[done]
    hist = np.zeros((256, 27), np.int64)
    np.add.at(hist, (cfg.reshape(-1), np.broadcast_to(CELL_CLASS, cfg.shape).reshape(-1)), 1)
    return hist


def own_projection(hist):
    """(256, 27) -> (256, 8): classes folded to (i == 0) << 2 | (j == 0) << 1 | (k == 0)."""
    out = np.zeros((256, 8), np.int64)
    for q, cl in enumerate(CLASSES):
        out[:, (cl[0] == 0) << 2 | (cl[1] == 0) << 1 | (cl[2] == 0)] += hist[:, q]
    return out


def seam_classes(mesh, vertex_offsets, model):
    """{(axis, copies)} over a mesh's input vertices (meshio.lattice_edges): copies is how many
    MPUs of the lattice hold the vertex's lattice edge, 1 for an edge inside an MPU, 2 on a face
    between two MPUs, 4 on the line where four meet; and the number of vertices on an MPU face
    (an off-axis lattice coordinate on a multiple of 7: what the weld counts as seam vertices)."""
    from parsip_amd import meshio

    g = meshio.lattice_edges(mesh, vertex_offsets, CS, *model.bbox)
    off_axis = np.arange(3)[None, :] != g[:, 3:4]
    hi = 7 * np.array(DIMS)[None, :]
    shared = (g[:, :3] % 7 == 0) & (g[:, :3] > 0) & (g[:, :3] < hi) & off_axis   # between two MPUs along that axis
    copies = 1 << shared.sum(axis=1)
    on_face = ((g[:, :3] % 7 == 0) & off_axis).any(axis=1)
    return set(zip(g[:, 3].tolist(), copies.tolist())), int(on_face.sum())
