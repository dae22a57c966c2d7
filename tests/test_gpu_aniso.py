"""Non-cubic MPU lattices through the HIP path (inputs: tests/aniso_util.py; their properties and
the oracle's standing on them: tests/test_aniso.py).  Every other device test runs a cube, where
dims[1] == dims[2] hides an exchanged pair in mpu_origin, the S1 brick decode, k_sieve, brick_box,
brick_layout, the live-list entries, the weld's lattice-edge keys, the group's seam weld and the
drop-in Polygonize's per-MPU bboxLo.  Here: lattices with three distinct dims or unit dims, each
shape in its three rotations, ragged ranges, through every launch shape, the sieve, the brick
spreading permutation (OPT_DEBUG bit 14), the weld, groups and the drop-in -- against the CPU
oracle bit for bit."""
import numpy as np
import pytest

import aniso_util as au
from parity_util import assert_bits_equal, assert_mesh_matches
from parsip_amd import gpu, meshio, soa, synth
from sieve_util import Sieve
from test_gpu_sieve import BEGIN, DEFAULTS, END, INFO, SEPARATE
from weld_util import check_contract, golden_counts

pytestmark = pytest.mark.gpu

RESET = {**DEFAULTS, gpu.OPT_DEBUG: 0, gpu.OPT_VERTEX_WIDE: 2, gpu.OPT_FINISH_QUAD: 2}
DIMS = list(au.LATTICES)
_ID = lambda d: "x".join(str(x) for x in d)  # noqa: E731
BOTH = gpu.LAUNCH_FRONT | gpu.LAUNCH_TREE_SPLIT
# name -> (options, flags that must be set with the generated kernels, flags that must not);
# the interpreter has neither k_front nor the split
SHAPES = {
    "separate": (SEPARATE, 0, BOTH),
    "front": ({gpu.OPT_FRONT: 1, gpu.OPT_TREE_SPLIT: 2, gpu.OPT_SPLIT_MAX_QUEUED: 0}, gpu.LAUNCH_FRONT, gpu.LAUNCH_TREE_SPLIT),
    "front_split": ({gpu.OPT_FRONT: 1, gpu.OPT_TREE_SPLIT: 1}, BOTH, 0),
}
_OM = {}


def _set(poly, opts):
    for k, v in opts.items():
        poly.set_option(k, v)


def oracle_mesh(oracle, key, model, cs, b, e):
    """The oracle's run of MPUs [b, e), computed once per ``key`` and left unchanged."""
    if (key, b, e) not in _OM:
        _OM[(key, b, e)] = oracle.polygonize(model, cs, b, e, threads=8)
    return _OM[(key, b, e)]


def run(poly, cs, b, e):
    info = poly.run(cs, b, e)
    return info, poly.download(), poly.stats()


def assert_runs_equal(a, b):
    (info1, mesh1, st1), (info0, mesh0, st0) = a, b
    for f in INFO:
        assert getattr(info1, f) == getattr(info0, f), f
    np.testing.assert_array_equal(st1, st0)
    for x in ("pos", "nrm", "col"):
        assert_bits_equal(getattr(mesh1, x), getattr(mesh0, x), x)
    np.testing.assert_array_equal(mesh1.tris, mesh0.tris)


# ---- every launch shape ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("jit", [0, 1])
@pytest.mark.parametrize("dims", DIMS, ids=_ID)
def test_named_lattice_every_launch_shape(gpu_poly, oracle, dims, jit, shape):
    model, cs = au.lattice_case(dims)
    n = int(np.prod(dims))
    opts, want, never = SHAPES[shape]
    if not jit:
        want, never = 0, BOTH
    try:
        _set(gpu_poly, {**RESET, **opts, gpu.OPT_JIT: jit})
        gpu_poly.set_model(model)
        assert gpu_poly.jit_active == bool(jit)
        info, mesh, st = run(gpu_poly, cs, 0, n)
    finally:
        _set(gpu_poly, RESET)
    assert info.ctMPUs == n
    assert info.launchFlags & want == want and not info.launchFlags & never, (shape, info.launchFlags)
    assert not info.launchFlags & gpu.LAUNCH_SIEVE
    assert_mesh_matches(mesh, st, oracle_mesh(oracle, dims, model, cs, 0, n))


# ---- ragged ranges ---------------------------------------------------------------------------
RANGE_DIMS = [(11, 5, 2), (2, 11, 5), (5, 2, 11), (1, 7, 4), (3, 6, 9)]


@pytest.mark.parametrize("name", list(au.RANGES[RANGE_DIMS[0]]))
@pytest.mark.parametrize("dims", RANGE_DIMS, ids=_ID)
def test_named_ranges(gpu_poly, oracle, dims, name):
    """The full lattice, a range from the middle of a z-row of an odd x-row to the middle of a
    later row, one inside an x-row, MPU 0 and the last MPU: the default launch shape and the
    separate launches, culling on and off."""
    model, cs = au.lattice_case(dims)
    b, e = au.RANGES[dims][name]
    om = oracle_mesh(oracle, dims, model, cs, b, e)
    try:
        gpu_poly.set_model(model)
        for opts in ({}, SEPARATE):
            for cull in (1, 0):
                _set(gpu_poly, {**RESET, **opts, gpu.OPT_CULLING: cull})
                info, mesh, st = run(gpu_poly, cs, b, e)
                assert info.ctMPUs == e - b
                if opts:
                    assert not info.launchFlags & gpu.LAUNCH_FRONT
                assert_mesh_matches(mesh, st, om)
    finally:
        _set(gpu_poly, RESET)


# ---- the sieve -------------------------------------------------------------------------------
SIEVE_CASES = [(d, "full") for d in DIMS] + [(d, "ragged") for d in ((11, 5, 2), (5, 2, 11), (3, 6, 9))]


@pytest.mark.parametrize("dims,name", SIEVE_CASES, ids=[f"{_ID(d)}-{n}" for d, n in SIEVE_CASES])
def test_sieve_on_named_lattices(gpu_poly, oracle, dims, name):
    """OPT_SIEVE 1: the mesh, the per-MPU stats and the run's counters are the unsieved run's and
    the oracle's, and the live list is the CPU model's live set, each brick once."""
    model, cs = au.lattice_case(dims)
    b, e = au.RANGES[dims][name]
    try:
        _set(gpu_poly, {**RESET, gpu.OPT_SIEVE: 1})
        gpu_poly.set_model(model)
        sieved = run(gpu_poly, cs, b, e)
        live = gpu_poly.live_bricks()
        gpu_poly.set_option(gpu.OPT_SIEVE, 0)
        plain = run(gpu_poly, cs, b, e)
    finally:
        _set(gpu_poly, RESET)
    assert sieved[0].launchFlags & gpu.LAUNCH_SIEVE and not plain[0].launchFlags & gpu.LAUNCH_SIEVE
    assert_mesh_matches(sieved[1], sieved[2], oracle_mesh(oracle, dims, model, cs, b, e))
    assert_runs_equal(sieved, plain)
    want_live = Sieve(model, cs, f"gpu_aniso_{_ID(dims)}").live_set(b, e)
    assert len(live) == len(want_live) and {tuple(int(x) for x in r) for r in live} == want_live


# ---- the brick-spreading permutation ---------------------------------------------------------
def _spread_case(which):
    if which == "C2":
        model, cs, _ = synth.make_config("C2")
        return model, cs, BEGIN, END
    model, cs = au.lattice_case(which)
    return (model, cs) + au.RANGES[which]["full"]


@pytest.mark.parametrize("front", [0, 1])
@pytest.mark.parametrize("which", [(3, 6, 9), (9, 3, 6), (11, 5, 2), "C2"], ids=lambda w: w if w == "C2" else _ID(w))
def test_brick_spreading(gpu_poly, oracle, which, front):
    """OPT_DEBUG bit 14 (bench.py --debug 16384): S1's wave W takes brick (W * stride) mod bricks.
    The mesh does not depend on which wave takes which brick."""
    model, cs, b, e = _spread_case(which)
    opts = {gpu.OPT_FRONT: 1, gpu.OPT_TREE_SPLIT: 2, gpu.OPT_SPLIT_MAX_QUEUED: 0} if front else SEPARATE
    try:
        _set(gpu_poly, {**RESET, **opts, gpu.OPT_DEBUG: gpu.DEBUG_BRICK_SPREAD})
        gpu_poly.set_model(model)
        info, mesh, st = run(gpu_poly, cs, b, e)
    finally:
        _set(gpu_poly, RESET)
    assert bool(info.launchFlags & gpu.LAUNCH_FRONT) == bool(front) and not info.launchFlags & gpu.LAUNCH_SIEVE
    assert_mesh_matches(mesh, st, oracle_mesh(oracle, which, model, cs, b, e))


def test_brick_spreading_under_the_sieve(gpu_poly, oracle):
    """With the sieve S1's waves take the live list: the permutation changes nothing there."""
    dims = (3, 6, 9)
    model, cs = au.lattice_case(dims)
    b, e = au.RANGES[dims]["full"]
    try:
        _set(gpu_poly, {**RESET, gpu.OPT_SIEVE: 1, gpu.OPT_DEBUG: gpu.DEBUG_BRICK_SPREAD})
        gpu_poly.set_model(model)
        spread = run(gpu_poly, cs, b, e)
        gpu_poly.set_option(gpu.OPT_DEBUG, 0)
        plain = run(gpu_poly, cs, b, e)
    finally:
        _set(gpu_poly, RESET)
    assert spread[0].launchFlags & plain[0].launchFlags & gpu.LAUNCH_SIEVE
    assert_mesh_matches(spread[1], spread[2], oracle_mesh(oracle, dims, model, cs, b, e))
    assert_runs_equal(spread, plain)


# ---- the fuzz trees in drawn boxes -----------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_fuzz_trees_in_drawn_boxes(gpu_poly, oracle, seed):
    """test_gpu_fuzz's trees and option draw, in boxes with three distinct dims."""
    model, cs, begin, end, cull, jit, (vwide, fquad, split) = au.fuzz_box_case(seed)
    front = (seed // 2) % 3
    try:
        _set(gpu_poly, {**RESET, gpu.OPT_CULLING: cull, gpu.OPT_JIT: jit, gpu.OPT_VERTEX_WIDE: vwide,
                        gpu.OPT_FINISH_QUAD: fquad,
                        gpu.OPT_TREE_SPLIT: (split if split or not front else 2) if jit else 0,
                        gpu.OPT_FUSED_SURFACE: seed % 4, gpu.OPT_FRONT: front})
        gpu_poly.set_model(model)
        assert gpu_poly.jit_active == bool(jit)
        info, mesh, st = run(gpu_poly, cs, begin, end)
    finally:
        _set(gpu_poly, RESET)
    assert_mesh_matches(mesh, st, oracle.polygonize(model, cs, begin, end, threads=8))


# ---- the device weld -------------------------------------------------------------------------
def _weld_input(which):
    if which == "weld_case":
        model, cs, _ = au.weld_case()
        return model, cs, 0, None
    dims, name = which
    model, cs = au.lattice_case(dims)
    return (model, cs) + au.RANGES[dims][name]


WELD_CASES = ["weld_case", ((3, 6, 9), "full"), ((6, 9, 3), "full"), ((3, 6, 9), "ragged")]


def weld_bytes(w):
    return tuple(np.ascontiguousarray(a).tobytes() for a in (w.pos, w.nrm, w.col, w.tris, w.vertex_map))


@pytest.mark.parametrize("which", WELD_CASES, ids=lambda w: w if isinstance(w, str) else f"{_ID(w[0])}-{w[1]}")
def test_weld_equals_host_definition(gpu_poly, which):
    """Polygonizer.weld() is byte-equal to meshio.weld_lattice of the same download (whose
    lattice-edge keys come from soa.mpu_origins and the same dims)."""
    model, cs, b, e = _weld_input(which)
    gpu_poly.set_model(model)
    info = gpu_poly.run(cs, b, e)
    mesh, w = gpu_poly.download(), gpu_poly.weld()
    ref, ref_map = meshio.weld_lattice(mesh, mesh.vertex_offsets, cs, *model.bbox, mpu_begin=b)
    assert w.info.ctInputVertices == info.ctVertices == len(mesh.pos) > 0
    assert (len(w.pos), len(w.tris)) == (w.info.ctVertices, w.info.ctTriangles) == (ref.n_vertices, ref.n_triangles)
    for what, got, want in (("pos", w.pos, ref.pos), ("nrm", w.nrm, ref.nrm), ("col", w.col, ref.col)):
        assert got.tobytes() == np.ascontiguousarray(want, np.float32).tobytes(), what
    assert np.array_equal(w.tris, ref.tris.astype(np.uint32))
    assert np.array_equal(w.vertex_map, ref_map.astype(np.uint32))
    check_contract(mesh.pos, mesh.nrm, mesh.col, mesh.tris, w, w.vertex_map)
    assert w.info.ctVertices < w.info.ctInputVertices  # seams were welded
    if which == "weld_case":
        gold = golden_counts()[au.WELD_CASE]
        assert (w.info.ctInputVertices, w.info.ctTriangles) == (gold["vertices"], gold["triangles"])
        assert w.info.ctVertices == gold["lattice_weld"]["vertices"] == 3378
        assert meshio.open_edge_count(w.tris) == gold["lattice_weld"]["open_edges"] == 0


# ---- groups ----------------------------------------------------------------------------------
_GROUPS = {}


@pytest.fixture(scope="module")
def groups():
    """k -> a Group of k parts on device 0 that splits however small the lattice is."""
    def get(k):
        if k not in _GROUPS:
            _GROUPS[k] = gpu.Group([0] * k)
            _GROUPS[k].set_option(gpu.GROUP_OPT_MIN_PART_MPUS, 0)
        return _GROUPS[k]

    yield get
    for g in _GROUPS.values():
        g.close()
    _GROUPS.clear()


def _group_input(which):
    if which == "weld_case":
        model, cs, _ = au.weld_case()
        return model, cs, soa.mpu_dims(cs, *model.bbox)
    return au.lattice_case(which) + (which,)


def _fixed_split(dims):
    """Five parts: a bound inside a z-row, an empty part, a bound on a z-row inside an x-slab,
    one between two slabs."""
    d0, d1, d2 = dims
    nyz = d1 * d2
    inside = nyz + 2 * d2 + d2 // 2
    bounds = [0, inside, inside, 3 * nyz + 2 * d2, 4 * nyz, d0 * nyz]
    assert inside % d2 and bounds[3] % d2 == 0 and bounds[3] % nyz and d0 > 4
    return bounds


@pytest.mark.parametrize("k", [2, 3, 8, "fixed"])
@pytest.mark.parametrize("which", ["weld_case", (9, 3, 6)], ids=lambda w: w if isinstance(w, str) else _ID(w))
def test_group_on_non_cubic_lattices(gpu_poly, oracle, groups, which, k):
    """The planned split into k parts and one fixed split: the group's download is the oracle's
    mesh, its weld the single context's byte for byte."""
    model, cs, dims = _group_input(which)
    n = int(np.prod(dims))
    om = oracle_mesh(oracle, which, model, cs, 0, n)
    gpu_poly.set_model(model)
    gpu_poly.run(cs)
    want = gpu_poly.weld()
    bounds = _fixed_split(dims) if k == "fixed" else None
    g = groups(5 if bounds else k)
    if bounds:
        g.set_split(bounds)
    g.set_model(model)
    total, parts = g.run(cs)
    if bounds:
        assert [(p.mpuBegin, p.mpuEnd) for p in parts] == list(zip(bounds[:-1], bounds[1:]))
    assert sum(1 for p in parts if p.info.ctMPUs) > 1 and sum(p.info.ctMPUs for p in parts) == n
    mesh = g.download()
    assert (total.ctMPUs, total.ctVertices, total.ctTriangles) == (n, len(om.pos), len(om.tris))
    np.testing.assert_array_equal(mesh.vertex_offsets, om.vertex_offsets)
    np.testing.assert_array_equal(mesh.triangle_offsets, om.triangle_offsets)
    assert_bits_equal(mesh.pos, om.pos, "positions")
    assert_bits_equal(mesh.nrm, om.nrm, "normals")
    assert_bits_equal(mesh.col, om.col, "colours")
    np.testing.assert_array_equal(mesh.local_tris(), om.tris)
    w = g.weld()
    assert weld_bytes(w) == weld_bytes(want)
    assert (w.info.ctVertices, w.info.ctSeamVertices) == (want.info.ctVertices, want.info.ctSeamVertices)
    if which == "weld_case":
        assert meshio.open_edge_count(w.tris) == 0 and w.info.ctVertices == 3378


# ---- the drop-in Polygonize ------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(5, 2, 11), (2, 11, 5)], ids=_ID)
def test_drop_in_polygonize(oracle, dims):
    """The bboxLo of the returned MPUs is soa.mpu_origins (the reference's, tests/test_aniso.py)
    bit for bit; counts and the first MPUs' vertices are the oracle's."""
    model, cs = au.lattice_case(dims)
    n = int(np.prod(dims))
    om = oracle_mesh(oracle, dims, model, cs, 0, n)
    rc, ct, mpus = gpu.Polygonize(cs, model, np.zeros(n, soa.MPU_DTYPE))
    assert rc == soa.RET_SUCCESS and ct == n
    assert_bits_equal(mpus["bboxLo"][:ct], soa.mpu_origins(cs, *model.bbox), "MPU origins")
    np.testing.assert_array_equal(mpus["ctVertices"][:ct], om.stats[:, 2])
    np.testing.assert_array_equal(mpus["ctTriangles"][:ct], om.stats[:, 3])
    np.testing.assert_array_equal(mpus["ctFieldEvals"][:ct], om.stats[:, 1])
    voff = om.vertex_offsets
    for i in np.flatnonzero(om.stats[:, 2]):
        nv = om.stats[i, 2]
        assert_bits_equal(mpus["vPos"][i, :nv * 3].reshape(-1, 3), om.pos[voff[i]:voff[i] + nv], "vPos")
