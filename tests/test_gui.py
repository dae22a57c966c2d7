"""Compat mode ("GUI-path semantics"): ParsipHaptics' own polygonizer,
CParsipOptimized over a COMPACTBLOBTREE, on the MI355X library against its CPU
restatement (oracle/psgui.c).

CPU tests: the tree conversion (COMPACTBLOBTREE::convert), the oracle's own invariants,
the MC-table property the device's vertex-ownership rule rests on, the libm agreement of
the correctly rounded powf / cosf / sinf, and the consistency of the reference scene with
the one run the reference recorded (Distrib/ParsipHaptics_Release.csv).
GPU tests (-m gpu): bit-exact meshes, statistics and field probes on the reference's
train scene and on random trees with every supported node type.
"""
import os

import numpy as np
import pytest

import psgui
from gui_util import assert_gui_mesh_equal, assert_info_equal as _info_equal, bits, random_ext_tree, random_tree
from parsip_amd import blobtree as bt
from parsip_amd import gui, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "tests", "golden", "train_corrected.scene")
B = bt.BlobNodeType


@pytest.fixture(scope="module")
def train():
    root = scene.load_scene(SCENE)[0]
    code, tree = gui.compact_blobtree(root)
    assert code == 0
    return root, tree


# ---------------------------------------------------------------- CPU --------
def test_convert_train_scene(train):
    root, tree = train
    assert (tree.ct_prims, tree.ct_ops) == (95, 31)  # recursive_CountPrimitives / Operators
    assert len(tree.kids) == 125  # every node but the root is some operator's kid
    # pre-order operator ids: kids of op i that are operators have larger ids
    for i, o in enumerate(tree.ops):
        for k in tree.kids[o["kidStart"]:o["kidStart"] + o["ctKids"]]:
            if k >> 16:
                assert (k & 0xFFFF) > i
    # a matrix slot per primitive with a non-identity backward matrix (:266-283)
    assert len(tree.mtx) == 1 + int(np.count_nonzero(tree.prims["idxMtx"]))
    assert np.array_equal(tree.mtx[0]["r"], np.eye(4, dtype=np.float32))
    ricci = tree.ops[tree.ops["type"] == B.OP_RICCIBLEND]
    assert len(ricci) and np.all(ricci["params"][:, 1] == np.float32(1.0) / ricci["params"][:, 0])


def test_convert_errors():
    assert gui.compact_blobtree(None)[0] == gui.ERR_PARAM_ERROR
    bad = bt.Op(B.OP_UNION, bt.Point((0, 0, 0)), bt.BlobNode(B.PRIM_POLYGON))
    assert gui.compact_blobtree(bad)[0] == gui.ERR_NODE_NOT_RECOGNIZED
    bad = bt.Op(B.OP_UNION, bt.Op(B.OP_GRADIENTBLEND, bt.Point((0, 0, 0)), bt.Point((1, 0, 0))))
    assert gui.compact_blobtree(bad)[0] == gui.ERR_NODE_NOT_RECOGNIZED
    many = bt.Op(B.OP_BLEND, *[bt.Point((0.01 * i, 0, 0)) for i in range(1025)])
    assert gui.compact_blobtree(many)[0] == gui.ERR_KIDS_OVERFLOW


def test_mc_table_crossing_edges_are_listed():
    """The device numbers vertices by the first cell (loop order) that holds their edge: that
    needs every config's triangle list to name exactly its sign-change edges."""
    import psoracle

    tri = np.asarray(psoracle.tritable()).reshape(256, 16)
    c1, c2 = [0, 2, 0, 1, 4, 6, 4, 5, 0, 1, 2, 3], [1, 3, 2, 3, 5, 7, 6, 7, 4, 5, 6, 7]
    for cfg in range(256):
        crossing = {e for e in range(12) if ((cfg >> c1[e]) & 1) != ((cfg >> c2[e]) & 1)}
        assert {int(e) for e in tri[cfg] if e != -1} == crossing, cfg


def test_oracle_vertices_on_surface_and_closed(train):
    _, tree = train
    r = psgui.polygonize(tree, *tree.root_octree, 0.2, 0.5, threads=8)
    i = r.info
    assert i.ctVertices == len(r.pos) > 1000 and i.ctTriangles == len(r.tris)
    assert i.ctMPUs == i.ctIntersectedMPUs <= i.ctProcessedMPUs <= i.ctLatticeMPUs
    f, _ = psgui.field_values(tree, r.pos)
    converged = np.abs(f - 0.5) < 0.001
    assert converged.mean() > 0.97  # the rest ran out of the 8 Newton iterations (reference behaviour)
    # per MPU the triangles index that MPU's vertices only; normals are unit
    for m in np.nonzero(r.stats["ctTriangles"])[0][:50]:
        t = r.tris[r.mpu_t[m]:r.mpu_t[m + 1]]
        assert t.min() >= r.mpu_v[m] and t.max() < r.mpu_v[m + 1]
    # unit normals, or normalizeXYZ's (1, 1, 1) where Newton ended on a flat field (:1072-1087)
    unit = np.isclose(np.linalg.norm(r.nrm, axis=1), 1.0, atol=1e-5)
    assert np.all(unit | np.all(r.nrm == 1.0, axis=1)) and unit.mean() > 0.97
    assert i.ctFieldEvals == int(r.stats["fieldEvals"].sum())
    assert i.ctCellsInIntersectedMPUs == 343 * i.ctIntersectedMPUs


def test_correctly_rounded_libm_against_glibc(train):
    """The documented deviation (oracle/psgui.c header): Ricci's powf and the warps' cosf / sinf
    are the correctly rounded fp32 results on both sides.  The host libm the reference would
    link differs from them by at most 1 ulp, on a small share of this scene's arguments (Ricci:
    kid fields in [0, 1] to the powers 2, 16, 20 and back) and of random angles."""
    _, tree = train
    r = psgui.polygonize(tree, *tree.root_octree, 0.25, 0.5, threads=8)
    ricci = tree.ops[tree.ops["type"] == B.OP_RICCIBLEND]
    f = np.concatenate([np.linspace(0, 1, 20001, dtype=np.float32), np.abs(r.pos[:, 0] % 1)]).astype(np.float32)
    n_pow, n = 0, 0
    for nn, inv in ricci["params"][:, :2]:
        for e in (nn, inv):
            d, u = psgui.libm_agreement(f, np.full(len(f), e, np.float32))
            assert u[0] <= 1, (e, u)
            n_pow += int(d[0])
            n += len(f)
    ang = np.random.default_rng(1).uniform(-8, 8, 200000).astype(np.float32)
    d, u = psgui.libm_agreement(ang, ang)
    assert u[1] <= 1 and u[2] <= 1, u
    assert n_pow / n < 0.01 and d[1] / len(ang) < 0.03 and d[2] / len(ang) < 0.03, (n_pow / n, d)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_oracle_random_trees_convert_and_run(seed):
    code, tree = gui.compact_blobtree(random_tree(seed))
    assert code == 0
    r = psgui.polygonize(tree, *tree.root_octree, 0.08, 0.5, threads=8)
    assert r.info.ctTriangles > 0 and np.all(np.isfinite(r.pos))


def test_reference_csv_consistency(train):
    """The only output the reference recorded for this path (Distrib/ParsipHaptics_Release.csv:2,
    95 prims, cellsize 0.13) came from a build with GRID_DIM 16 and a scene with 95 operators
    (train_corrected has 31): not a parity pin.  The restatement at GRID_DIM 16
    on the shipped scene stays within 2 % of its mesh and crossed-cell counts."""
    _, tree = train
    r = psgui.polygonize(tree, *tree.root_octree, 0.13, 0.5, threads=8, grid_dim=16)
    ref = {"faces": 146352, "vertices": 82370, "cells": 72620}
    got = {"faces": r.info.ctTriangles, "vertices": r.info.ctVertices, "cells": r.info.ctIntersectedCells}
    for k in ref:
        assert abs(got[k] - ref[k]) / ref[k] < 0.02, (k, got[k], ref[k])


def _outside_shell(rng, box, n):
    """n points in box widened by 25 % (at least 0.5) but outside box."""
    lo, hi = box[0].astype(np.float64), box[1].astype(np.float64)
    pad = np.maximum(0.25 * (hi - lo), 0.5)
    pts = rng.uniform(lo - pad, hi + pad, size=(4 * n, 3))
    out = ((pts < lo) | (pts > hi)).any(axis=1)
    return pts[out][:n].astype(np.float32)


def test_cull_boxes_are_conservative():
    """Outside a node's culling box the field is exactly +0 (oracle): single primitives of
    every type under random transforms and operators, and whole random trees outside the
    root operator's box."""
    rng = np.random.default_rng(11)
    checked = 0
    for seed in range(200):
        code, tree = gui.compact_blobtree(random_tree(100 + seed, n_prims=1 + seed % 4))
        assert code == 0
        pb, ob = gui.cull_boxes(tree)
        for box in list(pb) + [ob[0]]:
            if not np.isfinite(box).all() or (box[0] > box[1]).any():
                continue
            pts = _outside_shell(rng, box, 400)
            f, _ = psgui.field_values(tree, pts) if box is ob[0] else (None, None)
            if box is ob[0]:
                assert np.array_equal(bits(f), np.zeros(len(pts), np.uint32)), seed
                checked += 1
        # a single primitive: its own box bounds the tree's field
        if len(pb) == 1 and np.isfinite(pb[0]).all() and (pb[0][0] <= pb[0][1]).all():
            pts = _outside_shell(rng, pb[0], 400)
            f, _ = psgui.field_values(tree, pts)
            assert np.array_equal(bits(f), np.zeros(len(pts), np.uint32)), seed
            checked += 1
    assert checked > 40, checked


def _pcm_pair():
    """Two blobs in contact under a PCM: an operator kid and a primitive kid."""
    a = bt.Op(B.OP_BLEND, bt.Point((0, 0, 0)), bt.Point((0.3, 0, 0)),
              material=bt.Material(diffused=(1.0, 0.0, 0.0, 1.0)))
    a.children[1].material = bt.Material(diffused=(1.0, 0.5, 0.0, 1.0))
    b = bt.Point((0.55, 0.1, 0.0), material=bt.Material(diffused=(0.0, 0.0, 1.0, 1.0)))
    return bt.Op(B.OP_UNION, gui.Pcm(a, b, alpha_left=0.7, alpha_right=0.9))


def test_convert_pcm_and_instance():
    """COMPACTBLOBTREE::convert of PCM (params :168-177) and Instance (res1 :383-391, the
    compact id resolved by updateInstanceNodes :410-431)."""
    code, tree = gui.compact_blobtree(_pcm_pair())
    assert code == 0 and tree.ops[1]["type"] == B.OP_PCM
    w = np.float32(0.5) * np.float32(0.454202)  # PCM_PROPAGATION_WIDTH
    assert np.array_equal(tree.ops[1]["params"], np.array([w, w, 0.7, 0.9], np.float32))
    x = bt.Op(B.OP_BLEND, bt.Point((0, 0, 0)), bt.Point((0.3, 0, 0)))
    x.node_id = 17
    p = bt.Point((0, 0.5, 0))
    p.node_id = 23
    root = bt.Op(B.OP_UNION, bt.Instance(x), x, bt.Instance(p), p)
    code, tree = gui.compact_blobtree(root)
    assert code == 0
    inst = tree.prims[tree.prims["type"] == B.PRIM_INSTANCE]
    # origin x is operator 1, origin p is primitive 4 (DFS: inst, x's two points, inst, p)
    assert inst["res1"].tolist() == [[1.0, 17.0, 1.0, float(B.OP_BLEND)], [4.0, 23.0, 0.0, float(B.PRIM_POINT)]]


def test_oracle_pcm_contact_state_is_order_free():
    """The defined contact-state order (include/parsip_gpu_gui.h): a run reads the state it
    started with, so its mesh and the state it leaves do not depend on how the MPUs are
    split over threads (the reference's running maximum per TBB body does); the
    interpenetration raises the state above ISO_VALUE and the next run's propagation
    (a0 = alpha x state) then differs."""
    _, tree = gui.compact_blobtree(_pcm_pair())
    runs = [psgui.polygonize(tree, *tree.root_octree, 0.04, 0.5, threads=t) for t in (1, 3, 8)]
    for r in runs[1:]:
        assert_gui_mesh_equal(r, runs[0], "thread split")
        assert np.array_equal(r.pcm_state, runs[0].pcm_state)
    s1 = runs[0].pcm_state
    assert s1[0] > 0.5 and s1[1] > 0.5, s1
    r2 = psgui.polygonize(tree, *tree.root_octree, 0.04, 0.5, threads=8, pcm_state=s1)
    assert not (len(r2.pos) == len(runs[0].pos) and np.array_equal(bits(r2.pos), bits(runs[0].pos)))
    assert np.all(r2.pcm_state >= s1)
    # probes read the state and leave it alone; the propagation region sees it
    xyz = np.random.default_rng(3).uniform(*tree.root_octree, size=(4000, 3)).astype(np.float32)
    f1, _ = psgui.field_values(tree, xyz)
    f2, _ = psgui.field_values(tree, xyz, pcm_state=s1)
    assert 0 < np.count_nonzero(f1 != f2) < len(xyz)


def test_oracle_instance_is_its_origin_moved():
    """An Instance evaluates its origin at its backward-transformed point (:1069-1078): the
    field of Instance(x) translated by t at p equals x's field at p - t (to rounding)."""
    x = bt.Op(B.OP_RICCIBLEND, bt.Point((0, 0, 0)), bt.Line((0.2, 0, 0), (0.5, 0.3, 0)), n=2.0)
    t = np.array([1.0, 0.25, -0.5], np.float32)
    root = bt.Op(B.OP_UNION, x, bt.Instance(x, transform=bt.Affine((1, 1, 1), (0, 0, 0, 1), tuple(t))))
    _, tree = gui.compact_blobtree(root)
    _, solo = gui.compact_blobtree(bt.Op(B.OP_UNION, x))
    xyz = np.random.default_rng(4).uniform(-0.6, 0.9, size=(3000, 3)).astype(np.float32)
    f_inst, _ = psgui.field_values(tree, xyz + t)
    f_far, _ = psgui.field_values(solo, xyz + t)  # x's own field near the instance
    f_x, _ = psgui.field_values(solo, xyz)
    np.testing.assert_allclose(f_inst, np.maximum(f_x, f_far), atol=1e-5)
    assert np.count_nonzero(f_x > 0.5) > 100


def test_host_limits_of_pcm_and_instance():
    """set_tree's checks (PSGUI_RET_UNSUPPORTED / PARAM_ERROR), on the host through
    psgpu_gui_cull_boxes, and no generated kernels for these trees."""
    from parsip_amd import gpu

    def rc(root):
        code, tree = gui.compact_blobtree(root)
        assert code == 0
        try:
            gui.cull_boxes(tree)
            return 1
        except gpu.PsgpuError as e:
            return e.code

    pt = lambda x: bt.Point((x, 0, 0))  # noqa: E731
    assert rc(_pcm_pair()) == 1
    assert rc(bt.Op(B.OP_UNION, bt.Op(B.OP_PCM, pt(0), pt(0.3), pt(0.6)))) == gui.RET_UNSUPPORTED  # 3 kids
    nested = gui.Pcm(gui.Pcm(pt(0), pt(0.3)), pt(0.6))
    assert rc(bt.Op(B.OP_UNION, nested)) == gui.RET_UNSUPPORTED
    x = bt.Op(B.OP_BLEND, pt(0), pt(0.3))
    inner = bt.Op(B.OP_UNION, x, bt.Instance(x))
    assert rc(bt.Op(B.OP_UNION, inner, bt.Instance(inner))) == gui.RET_UNSUPPORTED  # nested instancing
    assert rc(bt.Op(B.OP_UNION, inner)) == 1
    pcm_x = gui.Pcm(pt(0), pt(0.3))
    assert rc(bt.Op(B.OP_UNION, pcm_x, gui.Pcm(pt(1), bt.Instance(pcm_x)))) == gui.RET_UNSUPPORTED
    _, tree = gui.compact_blobtree(bt.Op(B.OP_UNION, bt.Instance(pt(5)), pt(0)))  # origin outside the tree
    assert tree.prims["res1"][0][0] == -1.0
    with pytest.raises(gpu.PsgpuError) as e:
        gui.cull_boxes(tree)
    assert e.value.code == -1  # PSGPU_RET_PARAM_ERROR
    _, tree = gui.compact_blobtree(_pcm_pair())
    with pytest.raises(RuntimeError, match="-7"):
        gui.jit_compile(tree)


PCM_SCENE = """[Global]
NumLayers=1
RootIDs=(0)
[BLOBNODE 0]
IsOperator=1
OperatorType=UNION
ChildrenCount=3
ChildrenIDs=(1, 4, 5)
[BLOBNODE 1]
IsOperator=1
OperatorType=PCM
ChildrenCount=2
ChildrenIDs=(2, 3)
Propagate Left=0.3
Propagate Right=0.25
Attenuate Left=0.6
Attenuate Right=0.8
[BLOBNODE 2]
IsOperator=0
PrimitiveType=POINT
position=(0.0, 0.0, 0.0)
[BLOBNODE 3]
IsOperator=0
PrimitiveType=POINT
position=(0.5, 0.05, 0.0)
[BLOBNODE 4]
IsOperator=0
PrimitiveType=INSTANCE
OriginalNodeIndex=1
AffineTranslate=(1.5, 0.0, 0.0)
[BLOBNODE 5]
IsOperator=0
PrimitiveType=INSTANCE
OriginalNodeIndex=3
AffineTranslate=(0.0, 1.0, 0.0)
"""


def test_scene_pcm_and_instance():
    """The scene reader's PCM parameters (CPcm::loadScript) and INSTANCE origins
    (OriginalNodeIndex, findNodeByID), through convert and the oracle."""
    root = scene.load_scene(PCM_SCENE, from_text=True)[0]
    pcm, inst_op, inst_prim = root.children
    assert pcm.params == {"propagate_left": 0.3, "propagate_right": 0.25, "alpha_left": 0.6, "alpha_right": 0.8}
    assert inst_op.params["origin"] is pcm and inst_prim.params["origin"] is pcm.children[1]
    code, tree = gui.compact_blobtree(root)
    assert code == 0
    assert tree.prims["res1"][2].tolist() == [1.0, 1.0, 1.0, float(B.OP_PCM)]  # operator 1 (the root is 0)
    assert tree.prims["res1"][3].tolist() == [1.0, 3.0, 0.0, float(B.PRIM_POINT)]
    gui.cull_boxes(tree)  # the device's checks accept it
    r = psgui.polygonize(tree, *tree.root_octree, 0.05, 0.5, threads=8)
    assert r.info.ctTriangles > 0 and r.pcm_state[0] > 0.5
    with pytest.raises(scene.SceneError):
        scene.load_scene(PCM_SCENE.replace("OriginalNodeIndex=3", "OriginalNodeIndex=9"), from_text=True)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_oracle_random_ext_trees_run(seed):
    code, tree = gui.compact_blobtree(random_ext_tree(seed))
    assert code == 0
    assert np.any(tree.ops["type"] == B.OP_PCM) and np.any(tree.prims["type"] == B.PRIM_INSTANCE)
    r = psgui.polygonize(tree, *tree.root_octree, 0.1, 0.5, threads=8)
    assert r.info.ctTriangles > 0 and np.all(np.isfinite(r.pos))


@pytest.mark.parametrize("seed", [1, 2])
def test_jit_source_compiles_on_host(seed):
    """The generated compat kernels compile with hiprtc (no device needed)."""
    code, tree = gui.compact_blobtree(random_tree(seed))
    assert code == 0
    n, src = gui.jit_compile(tree)
    assert n > 10000 and "jit_gui_classify" in src and "prim_field_k" in src


# ---------------------------------------------------------------- GPU --------
# every GPU test runs on the interpreter kernels (jit 0) and on the tree's generated
# kernels (jit 2: set_tree waits for them), each with and without exact culling
@pytest.fixture(scope="module", params=[(0, 1), (2, 1), (0, 0), (2, 0)],
                ids=["interp", "jit", "interp-nocull", "jit-nocull"])
def gui_ctx(request):
    from parsip_amd import gpu

    gpu.load()
    assert gpu.device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"
    jit, cull = request.param
    p = gui.ParsipOptimized(0, jit=jit, cull=cull)
    p.jit_mode = jit
    yield p
    p.close()


def _expect_kernels(ctx):
    want = gui.JIT_ACTIVE if ctx.jit_mode == 2 else gui.JIT_NONE
    assert ctx.jit_status() == want


def _both(ctx, tree, cs, iso=0.5, octree=None):
    lo, hi = octree if octree is not None else tree.root_octree
    ctx.setup(tree, (lo, hi), 0, cs, iso)
    _expect_kernels(ctx)
    ctx.run()
    gm = ctx.exportMesh()
    om = psgui.polygonize(tree, lo, hi, cs, iso, threads=8)
    return gm, om


@pytest.mark.gpu
@pytest.mark.parametrize("cs", [0.25, 0.13])
def test_gpu_train_scene_bit_exact(gui_ctx, train, cs):
    _, tree = train
    gm, om = _both(gui_ctx, tree, cs)
    _info_equal(gui_ctx.finish(), om.info)
    assert_gui_mesh_equal(gm, om, f"train cs={cs}")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(1, 9))
def test_gpu_random_trees_bit_exact(gui_ctx, seed):
    code, tree = gui.compact_blobtree(random_tree(seed))
    assert code == 0
    gm, om = _both(gui_ctx, tree, 0.06)
    _info_equal(gui_ctx.finish(), om.info)
    assert_gui_mesh_equal(gm, om, f"seed {seed}")


@pytest.mark.gpu
def test_gpu_field_and_colour_probe(gui_ctx, train):
    _, tree = train
    gui_ctx.set_tree(tree)
    _expect_kernels(gui_ctx)
    lo, hi = tree.root_octree
    xyz = np.random.default_rng(5).uniform(lo, hi, size=(20000, 3)).astype(np.float32)
    gf, gc = gui_ctx.field_values(xyz)
    of, oc = psgui.field_values(tree, xyz)
    assert np.array_equal(bits(gf), bits(of)) and np.array_equal(bits(gc), bits(oc))
    assert np.count_nonzero(gf) > 1000


@pytest.mark.gpu
def test_gpu_isovalue_and_empty_lattice(gui_ctx, train):
    _, tree = train
    gm, om = _both(gui_ctx, tree, 0.3, iso=0.3)
    assert_gui_mesh_equal(gm, om, "iso 0.3")
    far = (np.array([100, 100, 100], np.float32), np.array([101, 101, 101], np.float32))
    gm, om = _both(gui_ctx, tree, 0.3, octree=far)
    assert len(gm.pos) == 0 and gui_ctx.finish().ctProcessedMPUs == 0 == om.info.ctProcessedMPUs


@pytest.mark.gpu
def test_gpu_rejects_unsupported_nodes(gui_ctx):
    pcm = bt.Op(B.OP_PCM, bt.Point((0, 0, 0)), bt.Point((0.5, 0, 0)), bt.Point((0.9, 0, 0)))  # 3 kids
    code, tree = gui.compact_blobtree(pcm)
    assert code == 0
    from parsip_amd import gpu

    with pytest.raises(gpu.PsgpuError) as e:
        gui_ctx.set_tree(tree)
    assert e.value.code == gui.RET_UNSUPPORTED


@pytest.mark.gpu
def test_gpu_structural_edit_does_not_wait():
    """A structural edit while the previous tree's kernels still compile returns at once (the
    old compile finishes in the background); the new tree's kernels then serve, bit-exact."""
    import time

    p = gui.ParsipOptimized(0, jit=1)
    try:
        _, tree_a = gui.compact_blobtree(random_tree(31, n_prims=14))
        _, tree_b = gui.compact_blobtree(random_tree(32, n_prims=14))
        t0 = time.perf_counter()
        p.set_tree(tree_a)
        p.set_tree(tree_b)
        assert time.perf_counter() - t0 < 2.0
        assert p.jit_status(wait=True) == gui.JIT_ACTIVE
        p.jit_mode = 2
        gm, om = _both(p, tree_b, 0.06)
        assert_gui_mesh_equal(gm, om, "after the edit")
    finally:
        p.close()


@pytest.mark.gpu
def test_gpu_run_polygonizer_api(train):
    root, _ = train
    p = gui.Run_Polygonizer(root, 0.25)
    V, T = p.statsMeshInfo()
    assert V > 0 and T > 0 and p.countMPUs() == p.statsIntersectedMPUs()
    assert p.statsTotalCellsInIntersectedMPUs() == 343 * p.statsIntersectedMPUs()
    p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["on_then_off", "off_then_on"])
def test_gpu_cull_toggle_between_set_tree_and_polygonize(order):
    """PSGUI_OPT_CULL changed after set_tree applies from the next set_tree: the kernels
    generated with (or without) culling boxes keep the box pointers they were built with, so
    turning culling off after a culling set_tree never hands them null boxes; bit-exact."""
    first = order == "on_then_off"
    p = gui.ParsipOptimized(0, jit=2, cull=first)
    p.jit_mode = 2
    try:
        _, tree = gui.compact_blobtree(random_tree(7, n_prims=10))
        p.set_tree(tree)
        assert p.jit_status() == gui.JIT_ACTIVE
        assert p._L.psgpu_gui_set_option(p._g, gui.OPT_CULL, int(not first)) == 1  # PSGPU_RET_SUCCESS
        gm, om = _both(p, tree, 0.06)
        assert_gui_mesh_equal(gm, om, f"cull toggled {order}")
        p.set_tree(tree)  # the new setting now applies; still bit-exact
        gm, om = _both(p, tree, 0.06)
        assert_gui_mesh_equal(gm, om, f"cull toggled {order}, after set_tree")
    finally:
        p.close()


# ---- PCM and Instance (the extended walk) ------------------------------------
def _ext_ctx(jit):
    from parsip_amd import gpu

    gpu.load()
    assert gpu.device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"
    return gui.ParsipOptimized(0, jit=jit)


def _ext_runs(p, tree, cs, runs=2):
    """`runs` polygonizations in a row on the device and on the oracle, each reading the
    contact state the previous one left: meshes, statistics and states bit-exact."""
    lo, hi = tree.root_octree
    p.setup(tree, (lo, hi), 0, cs, 0.5)
    assert p.jit_status() == gui.JIT_NONE  # no generated kernels for these trees
    state = np.array([0.5, 0.5], np.float32)
    assert np.array_equal(p.pcm_state, state)
    for k in range(runs):
        p.run()
        gm = p.exportMesh()
        om = psgui.polygonize(tree, lo, hi, cs, 0.5, threads=8, pcm_state=state)
        _info_equal(p.finish(), om.info)
        assert_gui_mesh_equal(gm, om, f"run {k}")
        state = om.pcm_state
        assert np.array_equal(p.pcm_state, state), (k, p.pcm_state, state)
    return state


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [0, 2])
def test_gpu_pcm_contact_bit_exact(jit):
    p = _ext_ctx(jit)
    try:
        _, tree = gui.compact_blobtree(_pcm_pair())
        state = _ext_runs(p, tree, 0.04, runs=3)
        assert state[0] > 0.5 and state[1] > 0.5
        # a new set_tree (= convert) starts from ISO_VALUE again
        p.set_tree(tree)
        assert np.array_equal(p.pcm_state, np.array([0.5, 0.5], np.float32))
    finally:
        p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(1, 7))
def test_gpu_random_ext_trees_bit_exact(seed):
    p = _ext_ctx(2)
    try:
        code, tree = gui.compact_blobtree(random_ext_tree(seed))
        assert code == 0
        _ext_runs(p, tree, 0.07, runs=2)
    finally:
        p.close()


@pytest.mark.gpu
def test_gpu_kernel_sets_in_one_context():
    """One context through every kernel set in turn (the other tests make a context per
    configuration): interpreter, generated, the extended walk of a PCM tree, generated again
    (a module loaded after one was unloaded), and back to the interpreter by option alone.
    After each step the mesh, statistics and offsets, and a 257-point field / colour probe,
    are bit-exact with the oracle."""
    cs = 0.12
    xyz_rng = np.random.default_rng(12)
    p = _ext_ctx(0)

    def set_jit(mode):
        assert p._L.psgpu_gui_set_option(p._g, gui.OPT_JIT, mode) == 1  # PSGPU_RET_SUCCESS

    def probe(tree, what, state=None):
        xyz = xyz_rng.uniform(*tree.root_octree, size=(257, 3)).astype(np.float32)
        gf, gc = p.field_values(xyz)
        of, oc = psgui.field_values(tree, xyz, pcm_state=state)
        assert np.array_equal(bits(gf), bits(of)) and np.array_equal(bits(gc), bits(oc)), what
        assert np.count_nonzero(gf) > 0, what

    def step(tree, status, what):
        lo, hi = tree.root_octree
        p.setup(tree, (lo, hi), 0, cs, 0.5)
        assert p.jit_status() == status, what
        p.run()
        om = psgui.polygonize(tree, lo, hi, cs, 0.5, threads=8)
        assert om.info.ctLatticeMPUs >= 100 and om.info.ctTriangles > 0, what
        _info_equal(p.finish(), om.info)
        assert_gui_mesh_equal(p.exportMesh(), om, what)
        assert p.jit_status() == status, what
        probe(tree, what)

    try:
        _, tree_a = gui.compact_blobtree(random_tree(3, n_prims=12))
        # seed 5, not 4: seed 4's root octree is flat in y, its lattice at this cell size empty
        _, tree_b = gui.compact_blobtree(random_tree(5, n_prims=12))
        _, tree_pcm = gui.compact_blobtree(_pcm_pair())
        p.set_tree(tree_a)
        step(tree_a, gui.JIT_NONE, "1: interpreter")
        set_jit(2)
        p.set_tree(tree_a)  # the same tree again: its kernels compile, set_tree waits for them
        step(tree_a, gui.JIT_ACTIVE, "2: generated")
        state = _ext_runs(p, tree_pcm, 0.03, runs=2)  # 240 MPUs; asserts JIT_NONE: the extended walk
        assert state[0] > 0.5 and state[1] > 0.5
        probe(tree_pcm, "3: extended", state=state)
        step(tree_b, gui.JIT_ACTIVE, "4: generated again")
        set_jit(0)
        step(tree_b, gui.JIT_NONE, "5: interpreter by option")
    finally:
        p.close()


@pytest.mark.gpu
def test_gpu_ext_probe_reads_state():
    p = _ext_ctx(0)
    try:
        _, tree = gui.compact_blobtree(random_ext_tree(4))
        p.set_tree(tree)
        xyz = np.random.default_rng(8).uniform(*tree.root_octree, size=(20000, 3)).astype(np.float32)
        for state in ([0.5, 0.5], [0.93, 1.4]):
            p.set_pcm_state(state)
            gf, gc = p.field_values(xyz)
            of, oc = psgui.field_values(tree, xyz, pcm_state=state)
            assert np.array_equal(bits(gf), bits(of)) and np.array_equal(bits(gc), bits(oc)), state
            assert np.array_equal(p.pcm_state, np.array(state, np.float32))  # probes leave it
        assert np.count_nonzero(gf) > 1000
    finally:
        p.close()


@pytest.mark.gpu
def test_gpu_instance_scene_bit_exact():
    """Instances of an operator and of a primitive beside their origins (and the colours
    they take from them), under transforms."""
    x = bt.Op(B.OP_RICCIBLEND, bt.Point((0, 0, 0), material=bt.Material(diffused=(1, 0, 0, 1))),
              bt.Line((0.2, 0, 0), (0.5, 0.3, 0), material=bt.Material(diffused=(0, 1, 0, 1))), n=2.0)
    y = bt.Cube((0, -0.6, 0), 0.15, material=bt.Material(diffused=(0, 0, 1, 1)))
    root = bt.Op(B.OP_UNION, x, y,
                 bt.Instance(x, transform=bt.Affine((1.2, 0.8, 1.0), (0.0, 0.0, 0.38268343, 0.9238795), (0.9, 0.3, 0))),
                 bt.Op(B.OP_BLEND, bt.Instance(y, transform=bt.Affine((1, 1, 1), (0, 0, 0, 1), (0.5, -0.2, 0.1))),
                       bt.Point((0.8, -0.6, 0.0))))
    p = _ext_ctx(1)
    try:
        _, tree = gui.compact_blobtree(root)
        _ext_runs(p, tree, 0.03, runs=1)
    finally:
        p.close()
