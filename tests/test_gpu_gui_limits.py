"""The compat mode (psgpu_gui.hip, psgpu_gui_device.h) at its tree-size, depth and lattice
limits, bit-exact against its CPU restatement (oracle/psgui.c): meshes, per-MPU statistics,
offsets, PsGuiInfo and field / colour probes, NaNs canonical (gui_util.bits).

1. tree sizes around the live masks' 64- and 128-node words: 63 ... 129 and 300 primitives,
   63 ... 129 operators over 40 primitives (`nP > 128` and `nO > 128` each alone);
2. operator nesting of exactly PSGUI_MAX_DEPTH (32), 33 refused, and the extended walk with
   an Instance whose origin brings the stack to 32 frames;
3. a bare primitive as the tree (no operator);
4. one operator folding 64, 65 and 1,024 kids;
5. the same on the trees' generated kernels wherever hiprtc needs at most 30 s for them;
6. lattices of 1, 1,023, 1,024, 1,025, 2,048, 2,049 and 103^3 MPUs (the offsets scan's blocks
   and its carry loop), the lattice and cell-size errors;
7. one context's buffers through small, large, one-MPU, empty and zero-MPU lattices.

hiprtc times of the generated kernels, measured on the CPU with gui.jit_compile (one compile
per tree and culling setting): bare primitives 0.5 s, the 64- / 65-kid folds 1.9-2.6 s, the
depth-32 chain 3.4 s, 63 ... 129 operators 3.7-5.4 s, 63-65 primitives 6.7 s, 127-129
primitives 13.6 s: all of these also run on their generated kernels.  300 primitives take
81 s and the 1,024-kid BLEND 1,483 s: those run on the interpreter kernels only.

CPU oracle times (threads=8) are at most 0.6 s per case; the lattices of section 1 have 240
to 336 MPUs (cell sizes 0.1, 0.12 and 0.16 over the trees' root octrees).
"""
import functools
import os

import numpy as np
import pytest

import gui_limits_util as U
import psgui
from gui_util import assert_gui_mesh_equal, assert_info_equal, bits
from parsip_amd import blobtree as bt
from parsip_amd import gui, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "tests", "golden", "train_corrected.scene")
B = bt.BlobNodeType


def _cube(h):
    return np.full(3, -h, np.float32), np.full(3, h, np.float32)


# name: (tree builder, cell size, octree or None for the root's, (prims, ops, most kids, depth),
#        lattice dims, generated kernels too)
CASES = {
    "prims63": (lambda: U.prim_count_tree(63), 0.1, None, (63, 32, 4, 5), (7, 6, 6), True),
    "prims64": (lambda: U.prim_count_tree(64), 0.1, None, (64, 33, 4, 4), (7, 6, 6), True),
    "prims65": (lambda: U.prim_count_tree(65), 0.1, None, (65, 33, 4, 4), (8, 6, 5), True),
    "prims127": (lambda: U.prim_count_tree(127), 0.12, None, (127, 65, 4, 5), (8, 8, 5), True),
    "prims128": (lambda: U.prim_count_tree(128), 0.12, None, (128, 64, 4, 5), (7, 7, 6), True),
    "prims129": (lambda: U.prim_count_tree(129), 0.12, None, (129, 65, 4, 5), (8, 8, 5), True),
    "prims300": (lambda: U.prim_count_tree(300), 0.16, None, (300, 150, 4, 5), (7, 8, 6), False),
    "ops63": (lambda: U.op_count_tree(63), 0.1, None, (40, 63, 4, 6), (7, 7, 6), True),
    "ops64": (lambda: U.op_count_tree(64), 0.1, None, (40, 64, 4, 6), (7, 7, 6), True),
    "ops65": (lambda: U.op_count_tree(65), 0.1, None, (40, 65, 4, 6), (7, 7, 6), True),
    "ops127": (lambda: U.op_count_tree(127), 0.1, None, (40, 127, 4, 7), (7, 7, 6), True),
    "ops128": (lambda: U.op_count_tree(128), 0.1, None, (40, 128, 4, 7), (7, 7, 6), True),
    "ops129": (lambda: U.op_count_tree(129), 0.1, None, (40, 129, 4, 7), (7, 7, 6), True),
    "chain32": (lambda: U.depth_chain(32), 0.12, None, (33, 32, 2, 32), (6, 6, 3), True),
    "bare-point": (lambda: U.bare_prim("point"), 0.05, None, (1, 0, 0, 0), (3, 3, 3), True),
    "bare-cube": (lambda: U.bare_prim("cube"), 0.05, None, (1, 0, 0, 0), (5, 5, 5), True),
    "bare-cylinder": (lambda: U.bare_prim("cylinder"), 0.05, None, (1, 0, 0, 0), (8, 4, 4), True),
}
SIZE_CASES = [n for n in CASES if n.startswith(("prims", "ops"))]
BARE_CASES = [n for n in CASES if n.startswith("bare")]
NARY_KINDS = {"blend": (B.OP_BLEND, None), "union": (B.OP_UNION, None), "ricci2": (B.OP_RICCIBLEND, 2.0),
              "ricci3.5": (B.OP_RICCIBLEND, 3.5)}
for _n in (64, 65, 1024):
    for _k, (_kind, _rn) in NARY_KINDS.items():
        CASES[f"nary{_n}-{_k}"] = (functools.partial(U.nary_tree, _kind, _n, _rn), 0.15, _cube(2.5), (_n, 1, _n, 1),
                                   (5, 5, 5), _n < 1024)
# DIF / SMOOTHDIF: kid 0 (the grid's lower corner) less the 64 others, on a tighter grid so that
# its neighbours cut into it; the operator's own octree is kid 0's, so the lattice is given
for _k, _kind in (("dif", B.OP_DIF), ("smoothdif", B.OP_SMOOTHDIF)):
    CASES[f"nary65-{_k}"] = (functools.partial(U.nary_tree, _kind, 65, None, 1.5), 0.15, _cube(2.0), (65, 1, 65, 1),
                             (4, 4, 4), True)
NARY_CASES = [n for n in CASES if n.startswith("nary")]

# every GPU test names its kernels and culling setting: the interpreter (jit 0) or the tree's
# generated kernels (jit 2: set_tree waits for them), with and without exact culling
INTERP = [(0, 1), (0, 0)]
ALL4 = [(0, 1), (2, 1), (0, 0), (2, 0)]
CFG_ID = {(0, 1): "interp", (2, 1): "jit", (0, 0): "interp-nocull", (2, 0): "jit-nocull"}


def _params(names):
    return [pytest.param(n, cfg, id=f"{n}-{CFG_ID[cfg]}") for n in names
            for cfg in (ALL4 if CASES[n][5] else INTERP)]


@functools.lru_cache(maxsize=None)
def _tree(name):
    return U.convert(CASES[name][0]())


def _octree(name):
    o = CASES[name][2]
    return o if o is not None else _tree(name).root_octree


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The case's reference mesh: computed once, shared by every configuration, never changed."""
    lo, hi = _octree(name)
    return psgui.polygonize(_tree(name), lo, hi, CASES[name][1], 0.5, threads=8)


@functools.lru_cache(maxsize=None)
def _train():
    code, tree = gui.compact_blobtree(scene.load_scene(SCENE)[0])
    assert code == 0
    return tree


@functools.lru_cache(maxsize=None)
def _train_oracle(cs):
    tree = _train()
    return psgui.polygonize(tree, *tree.root_octree, cs, 0.5, threads=8)


def _probe_points(lo, hi, n=4099, seed=17, widen=1.5):
    """n points (4,099: the last wave is partial) over the box widened about its centre."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, h = 0.5 * (lo + hi), 0.5 * widen * (hi - lo)
    return np.random.default_rng(seed).uniform(c - h, c + h, size=(n, 3)).astype(np.float32)


# ---------------------------------------------------------------- CPU --------
@pytest.mark.parametrize("name", list(CASES))
def test_builders_shapes_lattices_and_oracle(name):
    """Each case's exact primitive, operator, kid and depth counts, its exact lattice, and a
    non-empty oracle mesh."""
    tree = _tree(name)
    _, cs, _, shape, dims, _ = CASES[name]
    assert U.tree_shape(tree) == shape
    lo, hi = _octree(name)
    assert U.lattice_dims(lo, hi, cs) == dims
    om = _oracle(name)
    assert list(om.info.dims) == list(dims) and om.info.ctLatticeMPUs == dims[0] * dims[1] * dims[2]
    assert om.info.ctTriangles > 100 and om.info.ctVertices == len(om.pos) > 100
    if name in SIZE_CASES:
        assert 100 <= om.info.ctLatticeMPUs <= 400
        pb, _ = gui.cull_boxes(tree)
        finite = np.isfinite(pb).all(axis=(1, 2))
        assert finite.mean() >= 0.5, finite.mean()  # culling with all-infinite boxes tests nothing
        out = _probe_points(lo, hi)
        inside_any = np.zeros(len(out), bool)
        for b in pb[finite]:
            inside_any |= ((out >= b[0]) & (out <= b[1])).all(axis=1)
        assert 200 < np.count_nonzero(~inside_any) and 500 < np.count_nonzero(inside_any)


def test_builders_mask_word_boundaries():
    """The size cases reach what they are for: the second mask word of the primitives and of
    the operators each alone, and each half of `nP > 128 || nO > 128` alone."""
    shapes = {n: CASES[n][3] for n in SIZE_CASES}
    assert sorted(s[0] for n, s in shapes.items() if n.startswith("prims")) == [63, 64, 65, 127, 128, 129, 300]
    assert sorted(s[1] for n, s in shapes.items() if n.startswith("ops")) == [63, 64, 65, 127, 128, 129]
    assert all(s[0] <= 64 for n, s in shapes.items() if n.startswith("ops"))  # om1 without pm1
    assert shapes["prims129"][0] > 128 >= shapes["prims129"][1]
    assert shapes["ops129"][1] > 128 >= shapes["ops129"][0]
    assert shapes["prims300"][0] > 128 and shapes["prims300"][1] > 128


def _rc(root):
    from parsip_amd import gpu

    tree = U.convert(root)
    try:
        gui.cull_boxes(tree)
        return 1
    except gpu.PsgpuError as e:
        return e.code


def test_builders_depth_limits_on_the_host():
    """validate's depth check through psgpu_gui_cull_boxes: 32 nested operators pass and 33 do
    not; an Instance at depth d of an origin of height h passes with d + h == 32 only."""
    assert U.tree_shape(U.convert(U.depth_chain(31)))[3] == 31
    assert _rc(U.depth_chain(32)) == 1
    assert U.tree_shape(U.convert(U.depth_chain(33)))[3] == 33
    assert _rc(U.depth_chain(33)) == gui.RET_UNSUPPORTED
    assert U.tree_shape(U.convert(U.depth_chain(12)))[3] == 12
    ok = U.convert(U.instance_chain(20, 12))
    assert U.tree_shape(ok)[3] == 20 and np.count_nonzero(ok.prims["type"] == B.PRIM_INSTANCE) == 1
    assert _rc(U.instance_chain(20, 12)) == 1
    assert _rc(U.instance_chain(21, 12)) == gui.RET_UNSUPPORTED
    assert _rc(U.instance_chain(19, 12)) == 1


def _innermost(tree):
    """The operator whose kids are the two core POINTs."""
    for i, o in enumerate(tree.ops):
        ks = tree.kids[int(o["kidStart"]):int(o["kidStart"]) + int(o["ctKids"])]
        if len(ks) == 2 and all(not int(k) >> 16 and tree.prims["type"][int(k)] == B.PRIM_POINT for k in ks):
            last = i
    return last


@pytest.mark.parametrize("which", ["chain32", "instance20+12"])
def test_builders_deepest_frame_reaches_the_root(which):
    """The value of the operator in the stack's last frame shows at the root: with its two
    primitives moved away the oracle's field changes at many probe points."""
    build = (lambda: U.depth_chain(32)) if which == "chain32" else (lambda: U.instance_chain(20, 12))
    tree, moved = U.convert(build()), U.convert(build())
    o = moved.ops[_innermost(moved)]
    for k in moved.kids[int(o["kidStart"]):int(o["kidStart"]) + 2]:
        moved.prims["pos"][int(k)][:3] += 50.0
    xyz = _probe_points(*tree.root_octree, n=20000, widen=1.0)
    f, _ = psgui.field_values(tree, xyz)
    g, _ = psgui.field_values(moved, xyz)
    assert np.count_nonzero(f != g) > 500 and np.count_nonzero(f > 0.5) > 1000


@pytest.mark.parametrize("name", BARE_CASES)
def test_builders_bare_primitive_outside_its_box(name):
    """A bare primitive converts to 1 primitive and no operator; outside its culling box the
    oracle's field is exactly +0 and the colour the primitive's."""
    tree = _tree(name)
    assert (tree.ct_prims, tree.ct_ops, len(tree.kids)) == (1, 0, 0)
    pb, _ = gui.cull_boxes(tree)
    assert np.isfinite(pb).all()
    xyz = _probe_points(pb[0][0], pb[0][1], widen=1.6)
    out = ~((xyz >= pb[0][0]) & (xyz <= pb[0][1])).all(axis=1)
    f, c = psgui.field_values(tree, xyz)
    assert np.count_nonzero(out) > 1000 and np.count_nonzero(~out) > 100 and np.count_nonzero(f) > 50
    assert not bits(f[out]).any()
    assert np.array_equal(c, np.tile(tree.prims["color"][0], (len(xyz), 1)))


@pytest.mark.parametrize("name", BARE_CASES)
def test_builders_bare_primitive_generated_early_out(name):
    """The generated kernels of a bare primitive hold their own early-out exactly when
    culling is on: the branch test_gpu_bare_primitive_bit_exact's outside waves take."""
    early = "if (!prim_live(T, 0u, x, y, z)) return 0.0f;"
    _, src = gui.jit_compile(_tree(name), cull=True)
    assert src.count(early) == 1 and "Frame F0" not in src
    _, src = gui.jit_compile(_tree(name), cull=False)
    assert early not in src


@pytest.mark.parametrize("n", list(U.LATTICE_DIMS))
def test_builders_lattices(n):
    """The explicit octrees give exactly n MPUs, and the three-POINT tree a surface in the
    first, the middle and the last of them."""
    dims = U.LATTICE_DIMS[n]
    lo, hi = U.lattice_octree(dims)
    assert dims[0] * dims[1] * dims[2] == n and U.lattice_dims(lo, hi, U.LATTICE_CS) == dims
    om = psgui.polygonize(U.convert(U.three_point_tree(dims)), lo, hi, U.LATTICE_CS, 0.5, threads=8)
    assert om.info.ctLatticeMPUs == n and list(om.info.dims) == list(dims)
    t = om.stats["ctTriangles"]
    assert t[0] > 0 and t[n // 2] > 0 and t[n - 1] > 0
    if n > 1 << 20:
        # the last MPU lies in a 1,024-MPU block past the first 1,024 blocks, after two MPUs
        # with vertices: its offsets need the carry of k_gui_scan_top's first round
        assert (n - 1) // 1024 >= 1024 and om.mpu_v[n - 1] > 0 and om.mpu_t[n - 1] > 0
        assert om.stats["ctVertices"][1024 * 1024:].sum() > 0
    om = psgui.polygonize(U.convert(U.one_point_tree(dims)), lo, hi, U.LATTICE_CS, 0.5, threads=8)
    assert om.stats["ctTriangles"][n // 2] > 0 and om.info.ctLatticeMPUs == n


# ---------------------------------------------------------------- GPU --------
@pytest.fixture(scope="module")
def ctxs():
    """The module's contexts, one per (jit, cull), made when first asked for."""
    from parsip_amd import gpu

    gpu.load()
    assert gpu.device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"
    made = {}

    def get(cfg):
        if cfg not in made:
            p = gui.ParsipOptimized(0, jit=cfg[0], cull=cfg[1])
            p.jit_mode = cfg[0]
            made[cfg] = p
        return made[cfg]

    yield get
    for p in made.values():
        p.close()


def _expect_kernels(ctx):
    """A generated kernel that failed to compile is a failure, never a fallback."""
    assert ctx.jit_status() == (gui.JIT_ACTIVE if ctx.jit_mode == 2 else gui.JIT_NONE)


def _assert_offsets_are_scans(gm):
    """Independently of the oracle: the offsets are the exclusive sums of the downloaded counts."""
    for off, name in ((gm.mpu_v, "ctVertices"), (gm.mpu_t, "ctTriangles")):
        want = np.concatenate([[0], np.cumsum(gm.stats[name].astype(np.int64))])
        assert np.array_equal(off, want), name


def _run_and_compare(ctx, tree, octree, cs, om, what):
    ctx.setup(tree, octree, 0, cs, 0.5)
    _expect_kernels(ctx)
    ctx.run()
    gm = ctx.exportMesh()
    assert_info_equal(ctx.finish(), om.info)
    assert_gui_mesh_equal(gm, om, what)
    _assert_offsets_are_scans(gm)
    return gm


def _run_case(ctx, name):
    return _run_and_compare(ctx, _tree(name), _octree(name), CASES[name][1], _oracle(name), name)


def _probe_and_compare(ctx, tree, xyz, what):
    gf, gc = ctx.field_values(xyz)
    of, oc = psgui.field_values(tree, xyz)
    assert np.array_equal(bits(gf), bits(of)), what
    assert np.array_equal(bits(gc), bits(oc)), what
    return gf, gc


@pytest.mark.gpu
@pytest.mark.parametrize("name,cfg", _params(SIZE_CASES))
def test_gpu_tree_sizes_bit_exact(ctxs, name, cfg):
    """Section 1.  Oracle times here: at most 0.3 s per case (240 to 336 MPUs)."""
    ctx = ctxs(cfg)
    _run_case(ctx, name)
    xyz = _probe_points(*_octree(name))
    gf, _ = _probe_and_compare(ctx, _tree(name), xyz, name)
    assert 200 < np.count_nonzero(gf) < len(xyz) - 200


@pytest.mark.gpu
@pytest.mark.parametrize("name,cfg", _params(["chain32"]))
def test_gpu_depth_32_bit_exact(ctxs, name, cfg):
    """Section 2: the frame stack filled to its last entry."""
    ctx = ctxs(cfg)
    _run_case(ctx, name)
    _probe_and_compare(ctx, _tree(name), _probe_points(*_octree(name)), name)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ALL4, ids=[CFG_ID[c] for c in ALL4])
def test_gpu_depth_33_refused_and_previous_tree_kept(ctxs, cfg):
    from parsip_amd import gpu

    ctx = ctxs(cfg)
    _run_case(ctx, "chain32")
    with pytest.raises(gpu.PsgpuError) as e:
        ctx.set_tree(U.convert(U.depth_chain(33)))
    assert e.value.code == gui.RET_UNSUPPORTED
    _expect_kernels(ctx)  # the previous tree's kernels still serve
    ctx.run()
    assert_gui_mesh_equal(ctx.exportMesh(), _oracle("chain32"), "after the refusal")
    _probe_and_compare(ctx, _tree("chain32"), _probe_points(*_octree("chain32"), seed=18), "after the refusal")


@pytest.mark.gpu
def test_gpu_instance_origin_fills_the_stack():
    """The extended walk: an Instance in the operator at depth 20 of an origin of height 12 --
    32 frames -- over two runs in a row; depth 21 is refused and the tree stays."""
    from parsip_amd import gpu

    p = gui.ParsipOptimized(0, jit=2)
    try:
        tree = U.convert(U.instance_chain(20, 12))
        lo, hi = tree.root_octree
        p.setup(tree, (lo, hi), 0, 0.12, 0.5)
        assert p.jit_status() == gui.JIT_NONE  # no generated kernels for these trees
        for k in range(2):
            p.run()
            om = psgui.polygonize(tree, lo, hi, 0.12, 0.5, threads=8)
            assert om.info.ctTriangles > 1000
            assert_info_equal(p.finish(), om.info)
            assert_gui_mesh_equal(p.exportMesh(), om, f"run {k}")
            assert np.array_equal(p.pcm_state, om.pcm_state)
        with pytest.raises(gpu.PsgpuError) as e:
            p.set_tree(U.convert(U.instance_chain(21, 12)))
        assert e.value.code == gui.RET_UNSUPPORTED
        _probe_and_compare(p, tree, _probe_points(lo, hi), "after the refusal")
    finally:
        p.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,cfg", _params(BARE_CASES))
def test_gpu_bare_primitive_bit_exact(ctxs, name, cfg):
    """Section 3: no operator.  Outside the primitive's box the value is exactly +0 (the
    generated kernels return there early) and the colour the primitive's."""
    ctx = ctxs(cfg)
    tree = _tree(name)
    _run_case(ctx, name)
    pb, _ = gui.cull_boxes(tree)
    xyz = _probe_points(pb[0][0], pb[0][1], widen=1.6)
    out = ~((xyz >= pb[0][0]) & (xyz <= pb[0][1])).all(axis=1)
    gf, gc = _probe_and_compare(ctx, tree, xyz, name)
    assert np.count_nonzero(out) > 1000 and not bits(gf[out]).any()
    assert np.array_equal(gc, np.tile(tree.prims["color"][0], (len(xyz), 1)))
    # a wave with every point outside the box, and one with a single point inside
    far = xyz[out][:128].copy()
    far[64] = 0.5 * (pb[0][0] + pb[0][1])
    gf, _ = _probe_and_compare(ctx, tree, far, name + " far waves")
    assert not bits(gf[:64]).any() and gf[64] > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("name,cfg", _params(NARY_CASES))
def test_gpu_nary_folds_bit_exact(ctxs, name, cfg):
    """Section 4: one operator over 64, 65 and 1,024 POINTs (125 MPUs at cell size 0.15; the
    DIF and SMOOTHDIF cases 64 MPUs)."""
    ctx = ctxs(cfg)
    _run_case(ctx, name)
    _probe_and_compare(ctx, _tree(name), _probe_points(*_octree(name), n=1027), name)


# ---- lattices and the offsets scan -----------------------------------------
def _lattice_runs(ctx, n):
    dims = U.LATTICE_DIMS[n]
    octree = U.lattice_octree(dims)
    for build in (U.one_point_tree, U.three_point_tree):
        tree = U.convert(build(dims))
        om = psgui.polygonize(tree, *octree, U.LATTICE_CS, 0.5, threads=8)
        gm = _run_and_compare(ctx, tree, octree, U.LATTICE_CS, om, f"{n} MPUs, {build.__name__}")
        assert len(gm.mpu_v) == n + 1 and gm.mpu_v[-1] == len(gm.pos) > 200
        if build is U.three_point_tree:
            assert gm.mpu_v[1] > 0 and gm.mpu_v[n - 1] < gm.mpu_v[n]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [n for n in U.LATTICE_DIMS if n < 1 << 20])
def test_gpu_lattice_block_boundaries(ctxs, n):
    """Section 6: lattices at the edges of the scan's 1,024-MPU blocks."""
    _lattice_runs(ctxs((0, 1)), n)


@pytest.mark.gpu
def test_gpu_lattice_beyond_the_scan_top_block():
    """103^3 = 1,092,727 MPUs: 1,068 block sums, the second round of k_gui_scan_top's carry
    loop.  About 2.2 GB of field cache: the context goes when the test ends."""
    p = gui.ParsipOptimized(0, jit=0)
    p.jit_mode = 0
    try:
        _lattice_runs(p, 1092727)
    finally:
        p.close()


LATTICE_ERRORS = {
    "over-2^24": (U.lattice_octree((257, 257, 257)), U.LATTICE_CS, -2),  # PSGPU_RET_NOT_ENOUGH_MEM
    "cs-zero": (None, 0.0, -1),                                          # PSGPU_RET_PARAM_ERROR
    "cs-negative": (None, -0.25, -1),
    "cs-nan": (None, float("nan"), -1),
}


def _train_again(ctx, cs=0.25):
    tree = _train()
    _run_and_compare(ctx, tree, tree.root_octree, cs, _train_oracle(cs), f"train {cs}")


@pytest.mark.gpu
@pytest.mark.parametrize("what", list(LATTICE_ERRORS))
def test_gpu_lattice_errors_leave_the_context_usable(ctxs, what):
    from parsip_amd import gpu

    assert U.lattice_dims(*U.lattice_octree((257, 257, 257)), U.LATTICE_CS) == (257, 257, 257) and 257 ** 3 > 1 << 24
    ctx = ctxs((0, 1))
    octree, cs, code = LATTICE_ERRORS[what]
    ctx.setup(_train(), octree, 0, cs, 0.5)
    with pytest.raises(gpu.PsgpuError) as e:
        ctx.polygonize()
    assert e.value.code == code
    _train_again(ctx)


def _degenerate_octree():
    return np.array([0.0, 0.25, 0.0], np.float32), np.array([1.0, 0.25, 1.0], np.float32)


def _assert_zero_mpu_result(ctx, om):
    gm = ctx.exportMesh()
    info = ctx.finish()
    assert_info_equal(info, om.info)
    assert info.ctLatticeMPUs == 0 and list(info.dims)[1] == 0
    assert len(gm.pos) == 0 and len(gm.tris) == 0 and len(gm.stats) == 0
    assert gm.mpu_v.tolist() == [0] and gm.mpu_t.tolist() == [0]  # mpuOffsets[0] == 0


@pytest.mark.gpu
def test_gpu_degenerate_octree_is_empty(ctxs):
    ctx = ctxs((0, 1))
    tree = _train()
    lo, hi = _degenerate_octree()
    ctx.setup(tree, (lo, hi), 0, 0.25, 0.5)
    ctx.run()
    _assert_zero_mpu_result(ctx, psgui.polygonize(tree, lo, hi, 0.25, 0.5, threads=8))
    _train_again(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [0, 1])
def test_gpu_buffer_reuse_sequence(jit):
    """Section 7: one context through small, large, one-MPU, empty, zero-MPU, large again and
    a 300-primitive tree, each step bit-exact.  With jit 1 the train scene's generated kernels
    come in before the second run (jit_status(wait=True)) and every later set_tree swaps
    back to the interpreter until its own are ready.  The 300-primitive tree's kernels take
    81 s to compile and closing a context waits for its compile, so the jit 1 sequence turns
    the generated kernels off before that last step."""
    p = gui.ParsipOptimized(0, jit=jit)
    try:
        train = _train()

        def step(tree, octree, cs, what, om=None):
            lo, hi = octree
            om = om if om is not None else psgui.polygonize(tree, lo, hi, cs, 0.5, threads=8)
            p.setup(tree, (lo, hi), 0, cs, 0.5)
            p.run()
            if om.info.ctLatticeMPUs == 0:
                _assert_zero_mpu_result(p, om)
                return om
            gm = p.exportMesh()
            assert_info_equal(p.finish(), om.info)
            assert_gui_mesh_equal(gm, om, what)
            _assert_offsets_are_scans(gm)
            return om

        step(train, train.root_octree, 0.25, "1: train 0.25", _train_oracle(0.25))
        if jit:
            assert p.jit_status(wait=True) == gui.JIT_ACTIVE
        else:
            assert p.jit_status() == gui.JIT_NONE
        big = step(train, train.root_octree, 0.13, "2: train 0.13", _train_oracle(0.13))
        assert big.info.ctLatticeMPUs == 3920
        one = (1, 1, 1)
        om = step(U.convert(U.one_point_tree(one)), U.lattice_octree(one), U.LATTICE_CS, "3: one MPU")
        assert om.info.ctLatticeMPUs == 1 and om.info.ctVertices > 200
        far = (np.array([100, 100, 100], np.float32), np.array([101, 101, 101], np.float32))
        om = step(train, far, 0.3, "4: far octree")
        assert om.info.ctLatticeMPUs > 0 and om.info.ctProcessedMPUs == 0 and om.info.ctVertices == 0
        om = step(train, _degenerate_octree(), 0.25, "5: zero MPUs")
        assert om.info.ctLatticeMPUs == 0
        step(train, train.root_octree, 0.13, "6: train 0.13 again", _train_oracle(0.13))
        if jit:
            assert p._L.psgpu_gui_set_option(p._g, gui.OPT_JIT, 0) == 1  # PSGPU_RET_SUCCESS
        step(_tree("prims300"), _octree("prims300"), CASES["prims300"][1], "7: 300 primitives", _oracle("prims300"))
    finally:
        p.close()
