"""Dense inputs: MPUs with over 512 and up to 1,344 vertices (tests/test_dense.py,
tests/test_gpu_dense.py; DESIGN.md §2 "Dense MPUs").

Blob primitives have field radius 1 and iso distance 0.454.  At cell size 1 a LINE skeleton
through lattice corners puts exactly those corners inside (field 1); the nearest corner off
the line is 0.707 away, where the field is 0.125.  With every op a UNION (max) the fields do
not add, so the inside set is the set of corners the skeletons pass through, and every
lattice edge between an inside and an outside corner carries a vertex.  The scene box is set
to [0, 7 dims cs] so the lattice corners are integers x cs and the MPU lattice is `dims`.

Every builder's oracle mesh is checked by `assert_dense` for what makes it a dense input, so
a change to synth cannot quietly turn it into an easy one.  The inputs must not go through
the compiled reference: it writes past its 512-entry per-MPU arrays.
"""
import numpy as np

from parsip_amd import soa, synth
from parsip_amd.soa import NodeType

CS = 1.0
# the 13 lattice directions up to sign: 3 axes, 6 face diagonals, 4 space diagonals
DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1),
        (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1),
        (1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1)]

_ORACLE = {}


def segments_model(name, segs, dims, cs=CS):
    """A UNION tree over one LINE (or POINT, where both ends coincide) per segment
    ((x0, y0, z0), (x1, y1, z1)) in lattice corners, over a `dims` MPU lattice at cell size cs."""
    assert 1 <= len(segs) <= soa.MAX_TREE_NODES
    model = soa.Model.empty(name)
    P = model.prims
    for i, (a, b) in enumerate(segs):
        a = np.asarray(a, np.float32) * np.float32(cs)
        b = np.asarray(b, np.float32) * np.float32(cs)
        if (a == b).all():
            synth.set_prim(model, i, NodeType.POINT, a)
        else:
            synth.set_prim(model, i, NodeType.LINE, a)
            P["dirX"][0, i], P["dirY"][0, i], P["dirZ"][0, i] = b
    P["ctPrims"][0] = len(segs)
    synth.build_balanced_ops(model, len(segs))
    model.ops["opType"][0, :model.ct_ops] = NodeType.UNION
    synth.prepare_boxes(model)
    P["bboxLo"][0] = (0.0, 0.0, 0.0)
    P["bboxHi"][0] = tuple(np.float32(7 * d) * np.float32(cs) for d in dims)
    assert soa.mpu_dims(cs, *model.bbox) == tuple(dims), soa.mpu_dims(cs, *model.bbox)
    return model


def checker(dims=(1, 1, 1), cs=CS):
    """A 3-D checkerboard: a corner is inside iff x + y + z is even.  Per z, the face diagonals
    y - x = c with c = z (mod 2), each one LINE from its first to its last corner in the box (a
    POINT where it is a single corner).  Every lattice edge of every MPU is crossed: V = 1,344
    (the architectural maximum, 21 full batches of 64) and T = 1,372 per MPU.
    (1,1,1): 60 primitives, (2,1,1): 88, (1,1,2): 112."""
    nx, ny, nz = (7 * d + 1 for d in dims)
    segs = []
    for z in range(nz):
        for c in range(-(nx - 1), ny):
            if (c - z) % 2:
                continue
            x0, x1 = max(0, -c), min(nx - 1, ny - 1 - c)
            segs.append(((x0, x0 + c, z), (x1, x1 + c, z)))
    return segments_model("checker%dx%dx%d" % tuple(dims), segs, dims, cs)


def zlines(cs=CS):
    """32 LINEs along z through the (x, y) with x + y even, one MPU: V = 896, T = 1,372 (a tree
    of C3's size, for the generated-kernel variants)."""
    segs = [((x, y, 0), (x, y, 7)) for x in range(8) for y in range(8) if (x + y) % 2 == 0]
    return segments_model("zlines", segs, (1, 1, 1), cs)


def randlines(seed, n=128, dims=(2, 2, 2), max_len=8, through_centre=0, cs=CS):
    """`n` segments over a `dims` MPU lattice: a random start corner, one of the 13 lattice
    directions, 0 to max_len steps (0: a POINT); a segment that leaves the box is redrawn.
    The first `through_centre` (<= 3) are the axis lines through the lattice's middle corner rows
    instead, which every MPU of a 2x2x2 lattice touches with a corner (S1 looks at an MPU's 8
    corners only, so a sparse draw can lose every MPU)."""
    rng = np.random.default_rng(seed)
    hi = np.array([7 * d for d in dims])
    mid = [7 * (d // 2) for d in dims]
    segs = []
    for a in range(through_centre):
        s, e = list(mid), list(mid)
        s[a], e[a] = 0, int(hi[a])
        segs.append((tuple(s), tuple(e)))
    while len(segs) < n:
        s = rng.integers(0, hi + 1)
        d = np.array(DIRS[int(rng.integers(0, len(DIRS)))])
        e = s + d * int(rng.integers(0, max_len + 1))
        if (e < 0).any() or (e > hi).any():
            continue
        segs.append((tuple(int(v) for v in s), tuple(int(v) for v in e)))
    return segments_model("randlines%d_%d" % (seed, n), segs, dims, cs)


def randlines32(seed=3):
    """The 32-primitive randlines of the generated-kernel matrix: 2 MPUs side by side in z, long
    segments, the three middle rows first."""
    return randlines(seed, n=32, dims=(1, 1, 2), max_len=14, through_centre=3)


def randlines_mixed(seed=2):
    """56 segments: the oracle flags MPUs 4 and 7 only, so the first overflow MPU is not the
    range's first and unflagged MPUs follow a flagged one."""
    return randlines(seed, n=56, through_centre=3)


def randlines_below(seed=17):
    """The boundary from below: fewer segments, so that no MPU passes 512 vertices or triangles
    (the export succeeds) while V stays in the hundreds."""
    return randlines(seed, n=BELOW_N, through_centre=3)


# Seeds chosen on the CPU oracle (numpy.random.default_rng, the draw order of randlines):
# per-MPU V / T: 29: 442-675 / 741-1,132, no NaN; 31: 459-608 / 726-1,050, NaN positions and
# normals (the root bracket hits fb == fa); 48: 496-593 / 814-1,067, NaN normals only.
# mixed (56 segments, seed 2): V 233-354, T 368-594, MPUs 4 and 7 flagged, no NaN.
# below (48 segments, seed 17): V 142-321, T 206-494, no MPU flagged, no NaN.
BELOW_N = 48
RAND_SEEDS = (29, 31, 48)
NAN_SEED = 31
RAND_NAMES = tuple("randlines%d" % s for s in RAND_SEEDS)

# name -> (builder, per-MPU (V, T) the oracle must give, or None for the randlines rules)
INPUTS = {
    "checker": (checker, (1344, 1372)),
    "checker2x1x1": (lambda: checker((2, 1, 1)), (1344, 1372)),
    "checker1x1x2": (lambda: checker((1, 1, 2)), (1344, 1372)),
    "zlines": (zlines, (896, 1372)),
    **{"randlines%d" % s: ((lambda s=s: randlines(s)), None) for s in RAND_SEEDS},
    "randlines32": (randlines32, None),
    "mixed": (randlines_mixed, None),
    "below": (randlines_below, None),
}
DENSE = [n for n in INPUTS if n != "below"]  # the oracle flags an overflow MPU in each of these
_MODELS = {}


def model_of(name):
    if name not in _MODELS:
        _MODELS[name] = INPUTS[name][0]()
    return _MODELS[name]


def oracle_mesh(oracle, name, begin=0, end=0xFFFFFFFF):
    """The IEEE oracle's mesh of a named input (computed once per process and range, shared,
    never modified), checked for what makes the input dense."""
    key = (name, begin, end)
    if key not in _ORACLE:
        om = oracle.polygonize(model_of(name), CS, begin, end, threads=1)
        for a in (om.stats, om.pos, om.nrm, om.col, om.tris):
            a.setflags(write=False)
        if (begin, end) == (0, 0xFFFFFFFF):
            assert_dense(name, om)
        _ORACLE[key] = om
    return _ORACLE[key]


def assert_dense(name, om):
    """The properties of the oracle's output that make `name` a dense input."""
    st = om.stats
    V, T = st[:, 2].astype(np.int64), st[:, 3].astype(np.int64)
    want = INPUTS[name][1]
    if want is not None:
        assert (st[:, 0] == 1).all() and (st[:, 1] == 128).all(), name
        assert [(int(v), int(t)) for v, t in zip(V, T)] == [want] * len(st), (name, V, T)
        assert not np.isnan(om.pos).any() and not np.isnan(om.nrm).any(), name
        assert T.max() - 1 >= 1024, name              # tlocal bit 10
        if want[0] > 1024:
            assert int(om.tris.max()) >= 1024, name   # the split v2 bit, v0 / v1 bit 10
    elif name in RAND_NAMES:
        assert len(st) == 8 and (st[:, 0] == 1).all() and (V > 0).all(), (name, st)
        assert int((T > 512).sum()) >= 6, (name, T)
        assert int((V > 512).sum()) >= 3, (name, V)
    elif name == "randlines32":
        assert len(st) == 2 and (st[:, 0] == 1).all() and (V > 0).all(), (name, st)
        assert (T > 512).any() or (V > 512).any(), (name, V, T)
    elif name == "mixed":
        assert st[:, 4].tolist() == [0, 0, 0, 0, 1, 0, 0, 1], (name, st[:, 4], V, T)
    elif name == "below":
        assert len(st) == 8 and (st[:, 0] == 1).all(), (name, st)
        assert not st[:, 4].any() and V.max() <= 512 and T.max() <= 512, (name, V, T)
        assert V.min() >= 100 and T.max() > 384, (name, V, T)  # in the hundreds, close under the limit
    np.testing.assert_array_equal(st[:, 4], ((V > 512) | (T > 512)).astype(st.dtype), err_msg=name)


def interior_open_edges(tris, pos, dims, cs=CS):
    """Open edges (meshio.open_edge_count's: used by exactly one triangle) of an indexed mesh
    that do not lie on a face of the box [0, 7 dims cs]: open seams inside the lattice."""
    t = np.asarray(tris).astype(np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    e.sort(axis=1)
    uniq, cnt = np.unique(e, axis=0, return_counts=True)
    open_e = uniq[cnt == 1]
    p = np.asarray(pos, np.float64)
    hi = np.array([7.0 * d * cs for d in dims])
    a, b = p[open_e[:, 0]], p[open_e[:, 1]]
    on_face = ((a == 0) & (b == 0)) | ((a == hi) & (b == hi))  # both ends on the same box face
    return int((~on_face.any(axis=1)).sum()), len(open_e)
