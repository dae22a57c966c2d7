"""The compat mode's weld on the host (DESIGN.md §6 "Compat weld"): `gui.lattice_edges`,
`gui.mpu_vertex_edges` and `meshio.weld_by_edges` on the CPU oracle's compat meshes
(oracle/psgui.py), against tests/golden/gui_weld_counts.json
(tests/golden/make_gui_weld_counts.py).  No device: the device side is tests/test_gpu_gui_weld.py."""
import numpy as np
import pytest

import psgui
from gui_weld_util import (CASES, ISO, bit_weld_unfiltered, degenerate_count, golden, lattice_dims, make_tree,
                           mpu_of_vertex, weld_figures)
from parsip_amd import gui, meshio, soa
from weld_util import make_case, u32

_CACHE = {}


def oracle_case(name):
    """(tree, cellsize, dims, oracle mesh, lattice edges), computed once and left unchanged."""
    if name not in _CACHE:
        tree, cs = make_tree(name)
        om = psgui.polygonize(tree, *tree.root_octree, cs, ISO, threads=8)
        dims = lattice_dims(tree, cs)
        edges = gui.lattice_edges(om, dims, tree.root_octree[0], cs, ISO, lambda p: psgui.field_values(tree, p)[0])
        _CACHE[name] = (tree, cs, dims, om, edges)
    return _CACHE[name]


def welded(name):
    key = ("weld", name)
    if key not in _CACHE:
        _, _, _, om, edges = oracle_case(name)
        _CACHE[key] = meshio.weld_by_edges(meshio.TriMesh(om.pos, om.tris.astype(np.int64), om.nrm, om.col), edges)
    return _CACHE[key]


def test_inputs_cover_the_tails_and_lattices():
    """Between them the inputs have V mod 4 = 0, 1, 2, 3, three lattices that are no cube and one
    mesh below one wavefront."""
    g = golden()["cases"]
    assert {c["vertices"] % 4 for c in g.values()} == {0, 1, 2, 3}
    assert sum(len(set(c["dims"])) > 1 for c in g.values()) == 3
    assert g["sphere_cs0.3"]["dims"] == [1, 1, 1] and g["sphere_cs0.3"]["vertices"] == 36


@pytest.mark.parametrize("name", list(CASES))
def test_lattice_edges_names_every_mpu(name):
    """`gui.lattice_edges` raises on no MPU (every MPU's count is the mesh's), the lattice is the
    oracle's, every edge lies inside its MPU and an MPU has one vertex per edge."""
    tree, cs, dims, om, edges = oracle_case(name)
    assert dims == tuple(om.info.dims) == tuple(golden()["cases"][name]["dims"])
    assert edges.shape == (len(om.pos), 4) and edges.dtype == np.int64
    m = mpu_of_vertex(om.mpu_v)
    ijk = np.stack([m // (dims[2] * dims[1]), (m // dims[2]) % dims[1], m % dims[2]], axis=1)
    local = edges[:, :3] - 7 * ijk
    assert local.min() >= 0 and local.max() <= 7 and set(np.unique(edges[:, 3])) <= {0, 1, 2}
    assert (local[np.arange(len(local)), edges[:, 3]] <= 6).all()  # the lower corner along the axis
    assert len(np.unique(np.concatenate([m[:, None], edges], axis=1), axis=0)) == len(edges)


def test_lattice_edges_refuses_another_field():
    """A field that is not the run's gives other counts: ValueError, never a guess."""
    tree, cs, dims, om, _ = oracle_case("sphere_cs0.13")
    with pytest.raises(ValueError):
        gui.lattice_edges(om, dims, tree.root_octree[0], cs, ISO,
                          lambda p: psgui.field_values(tree, p + np.float32(0.05))[0])
    with pytest.raises(ValueError):
        gui.lattice_edges(om, (dims[0], dims[1], dims[2] + 1), tree.root_octree[0], cs, ISO,
                          lambda p: psgui.field_values(tree, p)[0])


@pytest.mark.parametrize("name", list(CASES))
def test_weld_matches_golden(name):
    """Welded counts, open edges, shell counts and Euler characteristics equal the golden file;
    no welded triangle is degenerate; none is dropped."""
    gold = golden()["cases"][name]
    _, cs, _, om, edges = oracle_case(name)
    fig = weld_figures(om, edges, cs)
    for k in ("vertices", "triangles", "edge_weld", "bit_weld", "vertices_with_copy", "max_copies",
              "copies_bits_differ"):
        assert fig[k] == gold[k], (k, fig[k], gold[k])
    w, vmap = welded(name)
    assert degenerate_count(w.tris) == 0 == gold["edge_weld"]["degenerate"]
    assert w.n_triangles == len(om.tris)
    assert np.array_equal(w.tris, vmap[om.tris.astype(np.int64)])


@pytest.mark.parametrize("name", list(CASES))
def test_copies(name):
    """No welded vertex has more than 4 copies, nor two from one MPU; the representative is the
    first copy and hands on its attributes bit for bit; copies lie within the recorded bound
    (the measured maximum times 8, in cell sizes) of their representative."""
    _, cs, _, om, edges = oracle_case(name)
    w, vmap = welded(name)
    assert np.bincount(vmap, minlength=w.n_vertices).max() <= 4
    pairs = np.stack([vmap, mpu_of_vertex(om.mpu_v)], axis=1)
    assert len(np.unique(pairs, axis=0)) == len(pairs)
    first = np.full(w.n_vertices, len(vmap), np.int64)
    np.minimum.at(first, vmap, np.arange(len(vmap)))
    assert (np.diff(first) > 0).all()  # ordered by smallest input index
    for a, b in ((w.pos, om.pos), (w.nrm, om.nrm), (w.col, om.col)):
        assert np.array_equal(u32(a), u32(b[first]))
    assert w.col.shape[1] == 4
    d = np.linalg.norm(om.pos.astype(np.float64) - om.pos[first[vmap]].astype(np.float64), axis=1)
    bound = golden()["copy_distance_bound_cs"]
    print(f"{name}: max copy distance {d.max() / cs:.3e} cs, bound {bound:.3e} cs")
    assert d.max() <= bound * cs


def test_position_bit_weld_collapses_triangles():
    """Why the feature exists: `meshio.weld` (position bits) of the cs 0.13 sphere merges
    vertices of different edges that share their Newton start corner, and 212 triangles
    collapse; the lattice-edge weld of the same mesh collapses none."""
    _, _, _, om, _ = oracle_case("sphere_cs0.13")
    tm = meshio.TriMesh(om.pos, om.tris.astype(np.int64), om.nrm, om.col)
    assert bit_weld_unfiltered(tm) == (128, 212)
    assert degenerate_count(welded("sphere_cs0.13")[0].tris) == 0


def test_mpu_vertex_edges_of_a_plane():
    """One MPU cut by the plane x = 2.5: 64 x-edges from corner (2, j, k), in creation order
    (the first cell in loop order that holds the edge, then its table row's order)."""
    fv = np.where(np.arange(8)[:, None, None] <= 2, 1.0, 0.0).astype(np.float32) * np.ones((8, 8, 8), np.float32)
    e = gui.mpu_vertex_edges(fv, 0.5)
    assert e.shape == (64, 4) and (e[:, 0] == 2).all() and (e[:, 3] == 0).all()
    assert len(np.unique(e, axis=0)) == 64
    assert tuple(e[0]) in {(2, 0, 0, 0), (2, 0, 1, 0), (2, 1, 0, 0), (2, 1, 1, 0)}  # cell (2, 0, 0) owns all four
    assert len(gui.mpu_vertex_edges(np.zeros((8, 8, 8), np.float32), 0.5)) == 0
    assert len(gui.mpu_vertex_edges(np.full((8, 8, 8), 0.5, np.float32), 0.5)) == 0  # f > iso: 0.5 is outside


def _weld_lattice_before(mesh, vertex_offsets, cellsize, lo, hi, mpu_begin=0):
    """`meshio.weld_lattice` as it was before `weld_by_edges` was taken out of it."""
    pos = np.ascontiguousarray(mesh.pos, np.float32).reshape(-1, 3)
    tris_in = np.asarray(mesh.tris).astype(np.int64)
    g = meshio.lattice_edges(mesh, vertex_offsets, cellsize, lo, hi, mpu_begin)
    if len(pos) == 0:
        return meshio.TriMesh(pos, tris_in, mesh.nrm, mesh.col), np.zeros(0, np.int64)
    if max(soa.mpu_dims(cellsize, lo, hi)) * 7 >= 1 << 20:
        raise ValueError("lattice too large for the edge key")
    key = (((g[:, 0] << 20 | g[:, 1]) << 20 | g[:, 2]) << 2) | g[:, 3]
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first)
    remap = np.empty_like(order)
    remap[order] = np.arange(len(order))
    vertex_map = remap[inverse.reshape(-1)]
    keep = first[order]
    return (meshio.TriMesh(pos[keep], vertex_map[tris_in], None if mesh.nrm is None else np.asarray(mesh.nrm)[keep],
                           None if mesh.col is None else np.asarray(mesh.col)[keep]), vertex_map)


@pytest.mark.parametrize("name", ["C1", "rand1_0.13", "rand3_0.071_mpus_243_486", "rand3_0.071_box_6x7x5"])
def test_weld_lattice_unchanged_by_the_refactor(oracle, name):
    """`weld_lattice` of a hot-path oracle mesh (tests/test_weld.py's inputs): the same bytes and
    dtypes as the code it had before it called `weld_by_edges`; and `weld_by_edges` of
    `lattice_edges` is that weld."""
    model, cs, (b, e) = make_case(name)
    om = oracle.polygonize(model, cs, b, 0xFFFFFFFF if e is None else e, threads=8)
    m = meshio.TriMesh(om.pos, om.global_tris(), om.nrm, om.col)
    old, old_map = _weld_lattice_before(m, om.vertex_offsets, cs, *model.bbox, mpu_begin=b)
    new, new_map = meshio.weld_lattice(m, om.vertex_offsets, cs, *model.bbox, mpu_begin=b)
    by, by_map = meshio.weld_by_edges(m, meshio.lattice_edges(m, om.vertex_offsets, cs, *model.bbox, mpu_begin=b))
    for w, vm in ((new, new_map), (by, by_map)):
        for x, y in ((w.pos, old.pos), (w.nrm, old.nrm), (w.col, old.col), (w.tris, old.tris), (vm, old_map)):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    assert new.col.shape[1] == 3


def test_weld_by_edges_arguments():
    z3 = np.zeros((0, 3), np.float32)
    w, vm = meshio.weld_by_edges(meshio.TriMesh(z3, np.zeros((0, 3), np.int64), z3, np.zeros((0, 4), np.float32)),
                                 np.zeros((0, 4), np.int64))
    assert w.n_vertices == 0 and len(vm) == 0
    one = meshio.TriMesh(np.zeros((2, 3), np.float32), np.zeros((0, 3), np.int64))
    with pytest.raises(ValueError):
        meshio.weld_by_edges(one, np.zeros((1, 4), np.int64))
    with pytest.raises(ValueError):
        meshio.weld_by_edges(one, np.array([[0, 0, 1 << 20, 0], [0, 0, 0, 0]]))
    with pytest.raises(ValueError):
        meshio.weld_by_edges(one, np.array([[0, 0, 0, 3], [0, 0, 0, 0]]))


def test_symbols_exported():
    """The weld's C-ABI is part of the compat mode's symbol list."""
    for name in ("psgpu_gui_download_edges", "psgpu_gui_weld", "psgpu_gui_weld_device", "psgpu_gui_download_weld",
                 "psgpu_gui_weld_times", "psgpu_gui_weld_shells", "psgpu_gui_weld_shells_device",
                 "psgpu_gui_download_weld_shells", "psgpu_gui_weld_shells_times", "psgpu_gui_weld_filter",
                 "psgpu_gui_weld_filter_device", "psgpu_gui_download_weld_filter", "psgpu_gui_weld_filter_times"):
        assert name in gui.EXPORTED_SYMBOLS
    assert gui.OPT_TIMING == 3
