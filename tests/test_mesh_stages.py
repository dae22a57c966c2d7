"""The inputs of tests/test_gpu_mesh_stages.py reach the branches they are there for: the counts
of weld_util.TAIL_COUNTS and SCAN_COUNTS on the CPU oracle's meshes with meshio.weld_lattice,
and what those counts imply for the 16-byte tails and the scan's carry loop."""
import pytest

from parsip_amd import meshio
from weld_util import SCAN_COUNTS, SCAN_NAME, TAIL_COUNTS, make_case

BLOCK = 256


def oracle_counts(oracle, name):
    """(MPUs, run vertices, triangles, welded vertices)."""
    model, cs, (b, e) = make_case(name)
    om = oracle.polygonize(model, cs, b, 0xFFFFFFFF if e is None else e, threads=8)
    m = meshio.TriMesh(om.pos, om.global_tris(), om.nrm, om.col)
    w, _ = meshio.weld_lattice(m, om.vertex_offsets, cs, *model.bbox, mpu_begin=b)
    assert w.n_triangles == m.n_triangles
    return len(om.vertex_offsets) - 1, m.n_vertices, m.n_triangles, w.n_vertices


@pytest.mark.parametrize("name", list(TAIL_COUNTS))
def test_tail_case_counts(oracle, name):
    mpus, V, T, Vw = oracle_counts(oracle, name)
    assert mpus == int(name.rsplit("_", 1)[1])
    assert (V, T, Vw) == TAIL_COUNTS[name]


def test_tail_cases_cover_every_residue():
    """Run vertices (k_weld_emit, k_weld_map), triangles (k_filter_tris, k_weld_map) and welded
    vertices (k_filter_emit): each count takes every residue mod 4 over the cases.  3 n mod 4
    of a last block of n = count mod 256 elements runs over the residues with it."""
    for column in range(3):
        counts = [c[column] for c in TAIL_COUNTS.values()]
        assert {n % 4 for n in counts} == {0, 1, 2, 3}
        assert {3 * (n % BLOCK) % 4 for n in counts} == {0, 1, 2, 3}
    assert min(c[0] for c in TAIL_COUNTS.values()) < 64      # a mesh smaller than one wave


def test_scan_case_counts(oracle):
    """Weld, shells and filter each scan more than 256 block counts: blocks of run vertices,
    of welded vertices, of max(welded vertices, triangles)."""
    assert oracle_counts(oracle, SCAN_NAME) == SCAN_COUNTS
    _, V, T, Vw = SCAN_COUNTS
    blocks = [-(-n // BLOCK) for n in (V, Vw, max(Vw, T))]
    assert blocks == [495, 381, 759] and min(blocks) > BLOCK
