"""meshio.weld_lattice (the weld by lattice-edge identity, DESIGN.md §6 "Weld") on the CPU
oracle's meshes, against the counts of tests/golden/weld_counts.json
(tests/golden/make_weld_counts.py) and against meshio.weld (position bits)."""
import numpy as np
import pytest

from parsip_amd import meshio, soa
from weld_util import CASES, check_contract, golden_counts, make_case, u32

_CACHE = {}


def oracle_case(oracle, name):
    """(model, cellsize, mpu_begin, oracle mesh as a TriMesh, vertex offsets), computed once."""
    if name not in _CACHE:
        model, cs, (b, e) = make_case(name)
        om = oracle.polygonize(model, cs, b, 0xFFFFFFFF if e is None else e, threads=8)
        _CACHE[name] = (model, cs, b, meshio.TriMesh(om.pos, om.global_tris(), om.nrm, om.col), om.vertex_offsets)
    return _CACHE[name]


def lattice_weld(oracle, name):
    key = ("weld", name)
    if key not in _CACHE:
        model, cs, b, m, voff = oracle_case(oracle, name)
        _CACHE[key] = meshio.weld_lattice(m, voff, cs, *model.bbox, mpu_begin=b)
    return _CACHE[key]


@pytest.mark.parametrize("name,vertices,open_bits", [("rand3_0.071", 3334, 1276), ("rand4_0.123457", 1654, 588),
                                                     ("rand3_0.071_box_6x7x5", 3378, 1032)])
def test_closed_surface_welds_watertight(oracle, name, vertices, open_bits):
    """A closed surface inside the box at an ordinary cell size: the lattice-edge weld leaves no
    open edge (every undirected edge in exactly two triangles), the weld by position bits
    leaves hundreds.  The third case is a (6, 7, 5) lattice, the others are cubes."""
    gold = golden_counts()[name]
    _, _, _, m, _ = oracle_case(oracle, name)
    w, _ = lattice_weld(oracle, name)
    assert gold["lattice_weld"] == {"vertices": vertices, "triangles": m.n_triangles, "open_edges": 0}
    assert (w.n_vertices, w.n_triangles) == (vertices, m.n_triangles)
    e = np.concatenate([w.tris[:, [0, 1]], w.tris[:, [1, 2]], w.tris[:, [2, 0]]])
    e.sort(axis=1)
    _, uses = np.unique(e, axis=0, return_counts=True)
    assert (uses == 2).all()
    assert meshio.open_edge_count(w.tris) == 0
    wb = meshio.weld(m)
    assert gold["bit_weld"] == {"vertices": wb.n_vertices, "open_edges": open_bits}
    assert meshio.open_edge_count(wb.tris) == open_bits


@pytest.mark.parametrize("name,vertices", [("C1", 1014), ("C2", 25143)])
def test_power_of_two_cellsize_equals_bit_weld(oracle, name, vertices):
    """At a power-of-two cell size both sides of a seam round a corner alike: the two welds give
    identical vertices, map and triangles."""
    _, _, _, m, _ = oracle_case(oracle, name)
    w, vm = lattice_weld(oracle, name)
    wb = meshio.weld(m)
    assert w.n_vertices == wb.n_vertices == vertices == golden_counts()[name]["lattice_weld"]["vertices"]
    assert wb.n_triangles == m.n_triangles  # the bit-weld dropped nothing, so the triangles line up
    for a, b in ((w.pos, wb.pos), (w.nrm, wb.nrm), (w.col, wb.col)):
        assert np.array_equal(u32(a), u32(b))
    assert np.array_equal(w.tris, wb.tris)
    key = u32(m.pos).reshape(-1, 3)
    _, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    assert np.array_equal(vm, rank[inverse.reshape(-1)])


@pytest.mark.parametrize("name", list(CASES))
def test_contract_and_golden_counts(oracle, name):
    """Every named input: no ambiguous vertex (weld_lattice raises on one), the contract of the
    map, and the committed counts."""
    gold = golden_counts()[name]
    _, _, _, m, _ = oracle_case(oracle, name)
    w, vm = lattice_weld(oracle, name)
    assert (m.n_vertices, m.n_triangles) == (gold["vertices"], gold["triangles"])
    assert gold["lattice_weld"] == {"vertices": w.n_vertices, "triangles": w.n_triangles,
                                    "open_edges": meshio.open_edge_count(w.tris)}
    check_contract(m.pos, m.nrm, m.col, m.tris, w, vm)


def test_ambiguity_guard():
    """A vertex exactly on a lattice corner has three exact coordinates: its edge cannot be told
    from positions alone, so weld_lattice raises; so it does on a vertex off every edge."""
    cs, lo, hi = 0.13, (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)
    org = soa.mpu_origins(cs, lo, hi, 5, 6)[0]
    step = np.float32(cs) * np.arange(8, dtype=np.float32)
    corner = np.array([[org[0] + step[3], org[1] + step[0], org[2] + step[7]]], np.float32)
    tris = np.zeros((0, 3), np.int64)
    with pytest.raises(ValueError, match="corner"):
        meshio.weld_lattice(meshio.TriMesh(corner, tris, corner, corner), [0, 1], cs, lo, hi, mpu_begin=5)
    on_edge = corner.copy()
    on_edge[0, 1] += np.float32(0.25 * cs)
    w, vm = meshio.weld_lattice(meshio.TriMesh(on_edge, tris, on_edge, on_edge), [0, 1], cs, lo, hi, mpu_begin=5)
    assert w.n_vertices == 1 and list(vm) == [0]
    off = on_edge.copy()
    off[0, 0] += np.float32(0.25 * cs)
    with pytest.raises(ValueError, match="not on a lattice edge"):
        meshio.weld_lattice(meshio.TriMesh(off, tris, off, off), [0, 1], cs, lo, hi, mpu_begin=5)


def test_sub_range_is_the_full_weld_restricted(oracle):
    """MPUs [243, 486) of the 729-MPU lattice: the weld of that run equals the full-range
    definition restricted to those MPUs' vertices (seams towards the other MPUs stay open)."""
    model, cs, _, full, voff = oracle_case(oracle, "rand3_0.071")
    assert len(voff) - 1 == 729
    _, full_map = lattice_weld(oracle, "rand3_0.071")
    _, _, b, sub, sub_off = oracle_case(oracle, "rand3_0.071_mpus_243_486")
    w, vm = lattice_weld(oracle, "rand3_0.071_mpus_243_486")
    v0, v1 = int(voff[243]), int(voff[486])
    assert b == 243 and sub.n_vertices == v1 - v0
    assert np.array_equal(u32(sub.pos), u32(full.pos[v0:v1]))
    # equal edges in the full lattice <=> equal ids in the full map; ranked by first occurrence
    _, first, inverse = np.unique(full_map[v0:v1], return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    assert np.array_equal(vm, rank[inverse.reshape(-1)])
    check_contract(sub.pos, sub.nrm, sub.col, sub.tris, w, vm)
    assert meshio.open_edge_count(w.tris) > 0
