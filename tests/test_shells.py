"""meshio.shells, the host form of psgpu_weld_shells (include/parsip_gpu.h, "shells of the
welded mesh"): hand-made meshes whose answers are exact in binary, the fixed-point sums against
plain float64 sums, and the CPU oracle's meshes against tests/golden/shell_counts.json
(tests/golden/make_shell_counts.py)."""
import numpy as np
import pytest

from parsip_amd import meshio
from shells_util import CASES, counts, cube, fan, golden_counts, integer_counts, make_case, two_cubes_interleaved

_CACHE = {}


def oracle_shells(oracle, name):
    """meshio.shells of the oracle's mesh welded by lattice-edge identity, and that weld; once."""
    if name not in _CACHE:
        model, cs, (b, e) = make_case(name)
        om = oracle.polygonize(model, cs, b, 0xFFFFFFFF if e is None else e, threads=8)
        m = meshio.TriMesh(om.pos, om.global_tris(), om.nrm, om.col)
        w, _ = meshio.weld_lattice(m, om.vertex_offsets, cs, *model.bbox, mpu_begin=b)
        _CACHE[name] = (meshio.shells(w), w)
    return _CACHE[name]


def only(sh):
    assert len(sh.shells) == sh.info["ctShells"] == 1
    return sh.shells[0]


def test_layouts():
    assert meshio.SHELL_DTYPE.itemsize == 72 and meshio.SHELLS_INFO_DTYPE.itemsize == 80
    assert meshio.SHELL_DTYPE.fields["area"][1] == 32 and meshio.SHELLS_INFO_DTYPE.fields["area"][1] == 40


def test_cube_is_exact():
    pos, tris = cube()
    sh = meshio.shells(pos, tris)
    s = only(sh)
    assert (s["firstVertex"], s["ctVertices"], s["ctTriangles"], s["ctEdges"], s["euler"]) == (0, 8, 12, 18, 2)
    assert (s["ctOpenEdges"], s["ctNonManifoldEdges"], s["ctFlippedEdges"]) == (0, 0, 0)
    assert s["area"] == 24.0 and s["volume"] == 8.0
    assert s["bboxLo"].tolist() == [-1.0] * 3 and s["bboxHi"].tolist() == [1.0] * 3
    info = sh.info
    assert (info["ctShells"], info["ctClosedShells"], info["ctEdges"], info["euler"]) == (1, 1, 18, 2)
    assert info["area"] == 24.0 and info["volume"] == 8.0
    assert not sh.vertex_shell.any() and not sh.tri_shell.any()
    assert meshio.shells(meshio.TriMesh(pos, tris)).tobytes() == sh.tobytes()


def test_cube_wound_inward_has_negative_volume():
    pos, tris = cube()
    sh = meshio.shells(pos, tris[:, ::-1])
    s = only(sh)
    assert s["area"] == 24.0 and s["volume"] == -8.0
    assert s["ctFlippedEdges"] == 0 and sh.info["ctClosedShells"] == 1


def test_cube_with_a_triangle_removed_is_open():
    pos, tris = cube()
    sh = meshio.shells(pos, tris[1:])
    s = only(sh)
    assert (s["ctTriangles"], s["ctEdges"], s["ctOpenEdges"], s["ctFlippedEdges"]) == (11, 18, 3, 0)
    assert sh.info["ctClosedShells"] == 0 and sh.info["ctOpenEdges"] == 3 == meshio.open_edge_count(tris[1:])


def test_cube_with_a_triangle_flipped():
    pos, tris = cube()
    tris[5] = tris[5, ::-1]
    sh = meshio.shells(pos, tris)
    s = only(sh)
    assert (s["ctFlippedEdges"], s["ctOpenEdges"], s["ctNonManifoldEdges"], s["euler"]) == (3, 0, 0, 2)
    assert sh.info["ctClosedShells"] == 0 and s["area"] == 24.0


def test_fan_has_one_non_manifold_edge():
    sh = meshio.shells(*fan())
    s = only(sh)
    assert (s["ctVertices"], s["ctTriangles"], s["ctEdges"]) == (5, 3, 7)
    assert (s["ctNonManifoldEdges"], s["ctOpenEdges"], s["ctFlippedEdges"]) == (1, 6, 0)


def test_two_interleaved_cubes():
    pos, tris = two_cubes_interleaved()
    sh = meshio.shells(pos, tris)
    assert sh.info["ctShells"] == sh.info["ctClosedShells"] == 2
    assert sh.shells["firstVertex"].tolist() == [0, 1]
    assert sh.vertex_shell.tolist() == [0, 1] * 8 and sh.tri_shell.tolist() == [0, 1] * 12
    assert (sh.vertex_shell[tris] == sh.tri_shell[:, None]).all()
    assert sh.shells["area"].tolist() == [24.0, 6.0] and sh.shells["volume"].tolist() == [8.0, 1.0]
    assert sh.shells["bboxLo"].tolist() == [[-1, -1, -1], [3.5, -0.5, -0.5]]
    assert sh.shells["bboxHi"].tolist() == [[1, 1, 1], [4.5, 0.5, 0.5]]
    assert sh.info["area"] == 30.0 and sh.info["volume"] == 9.0
    assert sh.info["bboxLo"].tolist() == [-1, -1, -1] and sh.info["bboxHi"].tolist() == [4.5, 1, 1]
    assert (sh.info["ctVertices"], sh.info["ctTriangles"], sh.info["ctEdges"], sh.info["euler"]) == (16, 24, 36, 4)


def test_unused_vertex_is_a_shell_of_its_own():
    pos, tris = cube()
    pos = np.concatenate([pos[:3], np.float32([[9, 9, 9]]), pos[3:]])   # vertex 3 is in no triangle
    tris = tris + (tris >= 3)
    sh = meshio.shells(pos, tris)
    assert sh.info["ctShells"] == 2 and sh.info["ctClosedShells"] == 1
    assert sh.shells["firstVertex"].tolist() == [0, 3]
    lone = sh.shells[1]
    assert (lone["ctVertices"], lone["ctTriangles"], lone["ctEdges"], lone["euler"]) == (1, 0, 0, 1)
    assert lone["area"] == 0.0 and lone["volume"] == 0.0 and lone["bboxLo"].tolist() == lone["bboxHi"].tolist() == [9, 9, 9]
    assert sh.vertex_shell.tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert sh.shells[0]["volume"] == 8.0


def test_empty_mesh_has_no_shell():
    sh = meshio.shells(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64))
    assert len(sh.shells) == len(sh.vertex_shell) == len(sh.tri_shell) == 0
    assert sh.info.tobytes() == bytes(80)


def test_a_degenerate_triangle_connects_but_has_no_loop_edge():
    pos = np.float32([[0, 0, 0], [1, 0, 0], [5, 5, 5]])
    sh = meshio.shells(pos, np.array([[0, 0, 1]]))
    s = sh.shells[0]   # edge 0-1 is used once each way: regular
    assert sh.info["ctShells"] == 2 and (s["ctVertices"], s["ctTriangles"], s["ctEdges"]) == (2, 1, 1)
    assert (s["ctOpenEdges"], s["ctFlippedEdges"], s["ctNonManifoldEdges"], s["area"]) == (0, 0, 0, 0.0)


def test_same_bytes_for_any_triangle_order(oracle):
    """The sums are integers: a permutation of the triangles changes no byte of the shells."""
    _, w = oracle_shells(oracle, "rand1_0.13")
    a = meshio.shells(w.pos, w.tris)
    perm = np.random.default_rng(5).permutation(len(w.tris))
    b = meshio.shells(w.pos, w.tris[perm])
    assert a.shells.tobytes() == b.shells.tobytes() and a.info.tobytes() == b.info.tobytes()
    assert np.array_equal(a.tri_shell[perm], b.tri_shell)


@pytest.mark.parametrize("name", ["C1", "rand1_0.13", "C2", "cube_minus_point"])
def test_fixed_point_sums_against_float64_sums(oracle, name):
    """Per shell and for the mesh, area and volume against plain float64 sums of the same terms,
    within 2 (n + 16) 2^-53 sum|term|, n the number of terms: the any-order summation bound
    plus the terms' own rounding, on both sides."""
    sh, w = oracle_shells(oracle, name)
    a2, v6 = meshio.shell_terms(w.pos, w.tris)
    groups = [(sh.shells[s], sh.tri_shell == s) for s in range(len(sh.shells))] + [(sh.info, np.ones(len(a2), bool))]
    for rec, sel in groups:
        n = int(sel.sum())
        for field, terms, div in (("area", a2[sel], 2.0), ("volume", v6[sel], 6.0)):
            bound = 2.0 * (n + 16) * 2.0 ** -53 * float(np.abs(terms).sum()) / div
            plain = float(terms.sum()) / div
            print(name, field, n, "fixed", float(rec[field]), "plain", plain, "bound", bound)
            assert abs(float(rec[field]) - plain) <= bound


def test_split_and_join_are_exact_on_binary_fractions():
    x = np.array([0.0, 1.0, -1.0, 0.75, -0.75, 2.0 ** -40, -(2.0 ** -40), 1234.5])
    for e in (0, 10, 45):
        hi, lo = meshio.shell_split(x, e)
        assert ((lo >= 0) & (lo < 1 << 30)).all()
        back = np.array([float(meshio.shell_join(h, l, e, 1.0)) for h, l in zip(hi, lo)])
        want = np.where(np.abs(x) * 2.0 ** (e + 30) >= 1.0, x, np.where(x < 0, -(2.0 ** (-e - 30)), 0.0))
        assert np.array_equal(back, want)


def test_scales():
    pos = np.float32([[0.5, -3.0, 1.0]])
    assert meshio.shell_scales(pos, 0) == (58 - 4 - 1, 58 - 6 - 1)           # M = 3 < 2^2, L = 1
    assert meshio.shell_scales(np.float32([[4.0, 0, 0]]), 5) == (58 - 6 - 3, 58 - 9 - 3)   # M = 4 < 2^3, L = 3
    assert meshio.shell_scales(np.float32([[0.25, 0, 0]]), 4) == (58 + 2 - 2, 58 + 3 - 2)  # M < 2^-1
    assert meshio.shell_scales(np.zeros((2, 3), np.float32), 2) == (57, 57)


@pytest.mark.parametrize("name", CASES)
def test_oracle_meshes_match_golden_counts(oracle, name):
    gold = golden_counts()[name]
    sh, w = oracle_shells(oracle, name)
    got = counts(sh)
    assert integer_counts(got) == integer_counts(gold)
    assert got["ctOpenEdges"] == meshio.open_edge_count(w.tris)
    assert got["ctFlippedEdges"] == 0
    assert (sh.vertex_shell[w.tris] == sh.tri_shell[:, None]).all()
    # measures: the oracle's positions may differ in their last bits between builds
    for g, s in zip([got] + got["per_shell"], [gold] + gold["per_shell"]):
        assert g["area"] == pytest.approx(s["area"], rel=1e-5, abs=1e-9)
        assert g["volume"] == pytest.approx(s["volume"], rel=1e-5, abs=1e-9)


# name -> (V, T, E, open, non-manifold, shells, euler) of the whole mesh
MESH_COUNTS = {
    "C1": (1014, 2024, 3036, 0, 0, 1, 2),
    "rand3_0.071": (3334, 6664, 9996, 0, 0, 1, 2),
    "rand4_0.123457": (1654, 3300, 4950, 0, 0, 2, 4),
    "rand1_0.13": (2503, 4868, 7371, 138, 0, 2, 0),
    "rand3_0.071_mpus_243_486": (2530, 4986, 7516, 74, 0, 1, 0),
    "rand3_0.071_box_6x7x5": (3378, 6752, 10128, 0, 0, 1, 2),
    "C2": (25143, 50034, 75175, 248, 0, 3, 2),
    "ring_union_point": (5980, 11984, 17975, 0, 1, 1, -11),
    "ring_point_apart": (5976, 11948, 17922, 0, 0, 2, 2),
    "cube_minus_point": (10662, 21316, 31974, 0, 0, 2, 4),
}


def test_golden_file_holds_the_known_counts():
    gold = golden_counts()
    assert sorted(gold) == sorted(CASES) == sorted(MESH_COUNTS)
    for name, want in MESH_COUNTS.items():
        g = gold[name]
        assert (g["ctVertices"], g["ctTriangles"], g["ctEdges"], g["ctOpenEdges"], g["ctNonManifoldEdges"],
                g["shells"], g["euler"]) == want, name
        assert g["ctFlippedEdges"] == 0
    per = {name: gold[name]["per_shell"] for name in gold}
    assert [s["firstVertex"] for s in per["rand4_0.123457"]] == [0, 403]
    assert [(s["firstVertex"], s["ctOpenEdges"]) for s in per["rand1_0.13"]] == [(0, 68), (60, 70)]
    assert [s["firstVertex"] for s in per["C2"]] == [0, 393, 5929]
    sliver = per["C2"][2]
    assert (sliver["ctVertices"], sliver["ctTriangles"], sliver["ctOpenEdges"], sliver["euler"]) == (6, 8, 0, 2)
    assert sliver["volume"] == pytest.approx(-8.19e-6, rel=1e-3)
    assert [s["euler"] for s in per["ring_point_apart"]] == [0, 2]
    cavity = per["cube_minus_point"][1]
    assert cavity["firstVertex"] == 4395 and cavity["volume"] == pytest.approx(-0.3877, rel=1e-3)
