"""Seeded inputs shared by the tests that pin the oracle and the HIP path to the compiled
reference (tests/test_reference.py, tests/test_gpu_reference.py) and by the generator of the
recorded reference outputs (tests/golden/make_reference_goldens.py)."""
import os

import numpy as np

from parsip_amd import soa, synth
from parsip_amd.soa import NodeType

# every primitive and operator the field function has a case for (= test_gpu_fuzz's TYPES / OPS)
ALL_TYPES = [NodeType.POINT, NodeType.LINE, NodeType.CYLINDER, NodeType.CUBE, NodeType.DISC, NodeType.RING,
             NodeType.TRIANGLE]
ALL_OPS = [NodeType.BLEND, NodeType.UNION, NodeType.INTERSECT, NodeType.DIF, NodeType.SMOOTHDIF,
           NodeType.RICCIBLEND, NodeType.GRADIENTBLEND, NodeType.WARPTWIST, NodeType.WARPTAPER,
           NodeType.WARPBEND, NodeType.WARPSHEAR]
# The reference evaluates Disc, Ring and RicciBlend with _mm_rsqrt_ps / _mm_rcp_ps
# (PS_Polygonizer.cpp:1116, :1158, :1292); every other node is plain IEEE arithmetic, so a tree
# without them has the same bits on every x86 CPU and in the IEEE oracle, normals excepted (:1619).
APPROX_TYPES = (NodeType.DISC, NodeType.RING)
APPROX_OPS = (NodeType.RICCIBLEND,)
# NULL (field 1 everywhere) empties most trees it appears in, so it is drawn less often
EXACT_TYPES = [NodeType.POINT, NodeType.LINE, NodeType.CYLINDER, NodeType.CUBE, NodeType.TRIANGLE] * 3 \
    + [NodeType.NULL]
EXACT_OPS = [o for o in ALL_OPS if o not in APPROX_OPS]
WARPS = (NodeType.WARPTWIST, NodeType.WARPTAPER, NodeType.WARPBEND, NodeType.WARPSHEAR)

GOLDEN_REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")
TYPE_NAMES = {v: k for k, v in vars(NodeType).items() if isinstance(v, int)}


def tree_case(seed, types=ALL_TYPES, ops=ALL_OPS, max_mpus=4096, matrices=None, n_max=24):
    """(model, cellsize): a random tree at a cell size off the round values, drawn so the
    [-2,2]^3 lattice has at most ``max_mpus`` MPUs.  ``matrices=None`` draws it per seed."""
    rng = np.random.default_rng(77000 + seed)
    n = int(rng.integers(2, n_max + 1))
    mats = bool(rng.integers(0, 2)) if matrices is None else matrices
    model = synth.random_model(77000 + seed, n_prims=n, types=types, op_types=ops, matrices=mats)
    per_axis = int(round(max_mpus ** (1.0 / 3)))
    assert per_axis ** 3 <= max_mpus
    # ceil(4 / cs) <= 7 * per_axis - 1 cells per axis
    lo = 4.0 / (7 * per_axis - 1.5)
    cs = float(np.float32(rng.uniform(lo, max(4.0 / 20, 1.5 * lo))))
    assert soa.count_mpus(cs, *model.bbox) <= max_mpus
    return model, cs


def node_types(model):
    """(sorted prim type codes, sorted op type codes) present in the tree."""
    p = sorted(set(int(t) for t in model.prims["skeletType"][0, :model.ct_prims]))
    o = sorted(set(int(t) for t in model.ops["opType"][0, :model.ct_ops]))
    return p, o


def has_approx(model) -> bool:
    p, o = node_types(model)
    return any(t in APPROX_TYPES for t in p) or any(t in APPROX_OPS for t in o)


def quads(model, cs, n_quads, seed):
    """S2-style sample points: ``n_quads`` groups of 4 consecutive lattice steps along z
    (x, y shared, z0 + k * cs) inside the scene box; returns x, y, z of length 4 * n_quads."""
    rng = np.random.default_rng(seed)
    lo, hi = model.bbox
    base = rng.uniform(lo, hi, (n_quads, 3)).astype(np.float32)
    csf = np.float32(cs)
    k = np.arange(4, dtype=np.float32)
    x = np.repeat(base[:, 0], 4)
    y = np.repeat(base[:, 1], 4)
    z = (base[:, 2:3] + k[None, :] * csf).astype(np.float32).reshape(-1)
    return x, y, z


def assert_oracle_mesh_equal(a, b, what, normals_atol=None, colours=True):
    """Two OracleMesh-shaped results (reference / oracle): every array bit-exact, normals
    optionally within a tolerance instead."""
    from parity_util import assert_bits_equal

    np.testing.assert_array_equal(a.stats[:, :4], b.stats[:, :4], err_msg=f"{what}: per-MPU passed/evals/V/T")
    np.testing.assert_array_equal(a.tris, b.tris, err_msg=f"{what}: triangles")
    assert_bits_equal(a.pos, b.pos, f"{what}: positions")
    if colours:
        assert_bits_equal(a.col, b.col, f"{what}: colours")
    if normals_atol is None:
        assert_bits_equal(a.nrm, b.nrm, f"{what}: normals")
    elif len(a.nrm):
        bad = ~(np.isclose(a.nrm, b.nrm, atol=normals_atol, rtol=0) | (np.isnan(a.nrm) & np.isnan(b.nrm)))
        assert not bad.any(), f"{what}: {np.count_nonzero(bad)} normal components beyond {normals_atol}"


# ---------------------------------------------------------------------------
# inputs of tests/test_reference.py (chosen once; the tests assert the properties they need)
SSE_SEEDS = range(100, 220)      # 2a: 120 trees over ALL_TYPES / ALL_OPS, 16 of them empty meshes
EXACT_SEEDS = range(300, 380)    # 2b: 80 trees over EXACT_TYPES / EXACT_OPS, 62 of them non-empty
BOX_SEEDS = range(100, 140)      # 2d: matrix-free trees over ALL_TYPES / ALL_OPS
N_QUADS = 100                    # 400 sample points per tree


def exact_case(seed, max_mpus=4096, n_max=24):
    return tree_case(seed, EXACT_TYPES, EXACT_OPS, max_mpus=max_mpus, n_max=n_max)


def _absdiff(a, b):
    """|a - b| with NaN against NaN counted as 0 and NaN against a number as inf."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    na, nb = np.isnan(a), np.isnan(b)
    d[na & nb] = 0.0
    d[na ^ nb] = np.inf
    d[(a == b)] = 0.0  # equal infinities
    return d


def _per_mpu(mesh):
    """Row of the owning MPU for every vertex."""
    return np.repeat(np.arange(len(mesh.stats)), mesh.stats[:, 2].astype(np.int64))


def measure_deviation(psref, psoracle, seeds=SSE_SEEDS):
    """How far the IEEE oracle (what the HIP path is held to) is from the compiled reference on
    the trees of ``seeds`` that hold a Disc, a Ring or a RicciBlend: the reference evaluates
    those with rsqrtps / rcpps, the oracle with correctly rounded 1/sqrt(x) and 1/x."""
    out = {"trees": 0, "trees_with_vt_difference": 0, "surface_mpus": 0, "mpus_vt_differ": 0,
           "field_max_abs": 0.0, "pos_max_abs": 0.0, "pos_max_abs_same_triangles": 0.0, "nrm_max_abs": 0.0}
    for s in seeds:
        model, cs = tree_case(s)
        if not has_approx(model):
            continue
        out["trees"] += 1
        x, y, z = quads(model, cs, N_QUADS, s)
        d = _absdiff(psoracle.field_value(model, x, y, z), psref.field_value(model, x, y, z))
        out["field_max_abs"] = max(out["field_max_abs"], float(d.max()))
        r = psref.polygonize(model, cs)
        o = psoracle.polygonize(model, cs, threads=8)
        assert len(r.stats) == len(o.stats)
        surface = (r.stats[:, 2] > 0) | (o.stats[:, 2] > 0)
        same = (r.stats[:, 2] == o.stats[:, 2]) & (r.stats[:, 3] == o.stats[:, 3])
        out["surface_mpus"] += int(surface.sum())
        out["mpus_vt_differ"] += int((~same).sum())
        out["trees_with_vt_difference"] += int((~same).any())
        rv, ov = same[_per_mpu(r)], same[_per_mpu(o)]
        if rv.any():
            out["pos_max_abs"] = max(out["pos_max_abs"], float(_absdiff(o.pos[ov], r.pos[rv]).max()))
            out["nrm_max_abs"] = max(out["nrm_max_abs"], float(_absdiff(o.nrm[ov], r.nrm[rv]).max()))
        # equal counts do not make equal meshes (a vertex may sit on another edge): the MPUs
        # whose triangle lists agree too show how far a vertex moves along its own edge
        rt, ot = r.triangle_offsets, o.triangle_offsets
        topo = same.copy()
        for i in np.flatnonzero(same & (r.stats[:, 3] > 0)):
            topo[i] = np.array_equal(r.tris[rt[i]:rt[i + 1]], o.tris[ot[i]:ot[i + 1]])
        rv, ov = topo[_per_mpu(r)], topo[_per_mpu(o)]
        if rv.any():
            out["pos_max_abs_same_triangles"] = max(out["pos_max_abs_same_triangles"],
                                                    float(_absdiff(o.pos[ov], r.pos[rv]).max()))
    out["mpu_vt_differ_share"] = out["mpus_vt_differ"] / max(1, out["surface_mpus"])
    return out


BOX_FIELDS_PRIMS = [f"vPrimBox{s}{c}" for s in ("Lo", "Hi") for c in "XYZ"] + ["bboxLo", "bboxHi"]
BOX_FIELDS_OPS = [f"vBox{s}{c}" for s in ("Lo", "Hi") for c in "XYZ"]


def measure_boxes(psref, psoracle, seeds=BOX_SEEDS):
    """Reference PrepareBBoxes against psoracle.prepare_bboxes on matrix-free trees.  Returns
    the max |difference| over the box fields, the most by which an oracle box lies inside the
    reference's, and the names of non-box fields whose bytes differ (must be none)."""
    out = {"trees": 0, "box_max_abs": 0.0, "oracle_inside_reference_max": 0.0, "non_box_fields_differing": []}
    for s in seeds:
        model, cs = tree_case(s, matrices=False)
        a, b = model.copy(), model.copy()
        assert psref.prepare_bboxes(a, cs) == 1 and psoracle.prepare_bboxes(b) == 1
        out["trees"] += 1
        for blk, boxf in (("prims", BOX_FIELDS_PRIMS), ("ops", BOX_FIELDS_OPS)):
            ra, rb = getattr(a, blk), getattr(b, blk)
            for f in ra.dtype.names:
                if f not in boxf:
                    if ra[f].tobytes() != rb[f].tobytes():
                        out["non_box_fields_differing"].append(f"{blk}.{f} seed {s}")
                    continue
                # slots past ctPrims / ctOps hold the shared input on both sides: difference 0
                va, vb = ra[f][0].astype(np.float64), rb[f][0].astype(np.float64)
                out["box_max_abs"] = max(out["box_max_abs"], float(_absdiff(va, vb).max()))
                inside = (vb - va) if "Lo" in f else (va - vb)
                out["oracle_inside_reference_max"] = max(out["oracle_inside_reference_max"], float(inside.max()))
        if a.mats.tobytes() != b.mats.tobytes() or a.boxmats.tobytes() != b.boxmats.tobytes():
            out["non_box_fields_differing"].append(f"matrices seed {s}")
    return out


# ---------------------------------------------------------------------------
# recorded reference outputs (tests/golden/reference/*.npz)
def model_from_bytes(prims, mats, ops, name="fixture"):
    m = soa.Model.empty(name)
    m.prims = np.frombuffer(bytes(prims), soa.PRIMS_DTYPE).copy()
    m.mats = np.frombuffer(bytes(mats), soa.PRIM_MATRICES_DTYPE).copy()
    m.ops = np.frombuffer(bytes(ops), soa.OPS_DTYPE).copy()
    return m


def fixture_names():
    import json

    with open(os.path.join(GOLDEN_REF, "index.json")) as f:
        return list(json.load(f)["fixtures"])


def load_fixture(name):
    """(model, cellsize, arrays, recorded mesh as an OracleMesh) of one recorded reference run."""
    from psoracle import OracleMesh

    with np.load(os.path.join(GOLDEN_REF, name + ".npz"), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    model = model_from_bytes(d["prims"], d["mats"], d["ops"], name)
    stats = np.zeros((len(d["evals"]), 5), np.uint32)
    stats[:, 0] = d["evals"] != 0
    stats[:, 1], stats[:, 2], stats[:, 3] = d["evals"], d["ctv"], d["ctt"]
    mesh = OracleMesh(0, stats, d["pos"], d["nrm"], d["col"], d["tris"])
    return model, float(d["cellsize"]), d, mesh
