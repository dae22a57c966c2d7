"""The dense inputs (tests/dense_util.py) on the CPU oracle: they are what they claim to be
(over 512, up to 1,344 vertices and 1,372 triangles per MPU), the oracle flags exactly the
MPUs past the reference's 512, its two builds agree on them, and the host weld closes every
seam between dense MPUs.  tests/test_gpu_dense.py compares the HIP path with these meshes."""
import numpy as np
import pytest

import dense_util as du
from parity_util import assert_bits_equal
from parsip_amd import meshio, soa
from weld_util import check_contract


@pytest.mark.parametrize("name", list(du.INPUTS))
def test_fixture_properties(oracle, name):
    """assert_dense on the oracle's output (exact counts of checker / zlines, the randlines
    thresholds, the boundary variant under the limit) and the overflow flag per MPU."""
    om = du.oracle_mesh(oracle, name)  # runs assert_dense
    V, T = om.stats[:, 2], om.stats[:, 3]
    np.testing.assert_array_equal(om.stats[:, 4] != 0, (V > 512) | (T > 512))
    assert om.stats[:, 4].any() == (name in du.DENSE)
    assert len(om.stats) == int(np.prod(soa.mpu_dims(du.CS, *du.model_of(name).bbox)))
    # MPU-local ids are a permutation-free cover: every vertex of an MPU is used by a triangle
    voff, toff = om.vertex_offsets, om.triangle_offsets
    for w in range(len(om.stats)):
        t = om.tris[toff[w]:toff[w + 1]]
        assert t.max() == V[w] - 1 and len(np.unique(t)) == V[w], (name, w)


def test_checker_counts_and_primitives(oracle):
    assert [du.model_of(n).ct_prims for n in ("checker", "checker2x1x1", "checker1x1x2", "zlines")] == [60, 88, 112, 32]
    for n in ("checker", "checker2x1x1", "checker1x1x2"):
        om = du.oracle_mesh(oracle, n)
        assert om.stats[:, 2:4].tolist() == [[1344, 1372]] * len(om.stats)
        assert int(om.tris.max()) == 1343
    assert du.oracle_mesh(oracle, "zlines").stats[0, 2:4].tolist() == [896, 1372]
    # the same counts at a cell size that is no power of two
    om = oracle.polygonize(du.checker(cs=0.75), 0.75)
    assert om.stats[:, 2:4].tolist() == [[1344, 1372]] and not np.isnan(om.pos).any()


def test_randlines_reach_local_ids_past_1024_and_a_nan_case(oracle):
    oms = [du.oracle_mesh(oracle, n) for n in du.RAND_NAMES]
    assert max(int(om.stats[:, 3].max()) for om in oms) - 1 >= 1024  # a triangle's local id: tlocal bit 10
    assert np.isnan(du.oracle_mesh(oracle, "randlines%d" % du.NAN_SEED).pos).any()


def test_checker_field_is_the_checkerboard(oracle):
    x, y, z = (a.reshape(-1).astype(np.float32) for a in np.meshgrid(*[np.arange(8)] * 3, indexing="ij"))
    f = oracle.field_value(du.model_of("checker"), x, y, z)
    np.testing.assert_array_equal(f >= 0.5, (x + y + z) % 2 == 0)
    assert set(np.unique(f).tolist()) <= {0.0, 0.125, 1.0}, np.unique(f)


@pytest.mark.parametrize("name", list(du.INPUTS))
def test_sse_and_ieee_builds_agree(oracle, name):
    """As test_oracle.py's test_sse_variant_normals_within_tolerance (UNION / LINE / POINT trees:
    no Disc, Ring or RicciBlend): stats, positions and triangles bit for bit, normals within 2e-3."""
    a = du.oracle_mesh(oracle, name)
    b = oracle.polygonize(du.model_of(name), du.CS, sse_approx=True)
    np.testing.assert_array_equal(a.stats, b.stats)
    assert_bits_equal(a.pos, b.pos, "positions")
    np.testing.assert_array_equal(a.tris, b.tris)
    assert_bits_equal(a.col, b.col, "colours")
    np.testing.assert_array_equal(np.isnan(a.nrm), np.isnan(b.nrm))
    if len(a.nrm):
        assert np.nanmax(np.abs(a.nrm - b.nrm)) <= 2e-3


@pytest.mark.parametrize("name", ["randlines%d" % du.RAND_SEEDS[0], "below", "checker2x1x1", "checker1x1x2"])
def test_weld_lattice_closes_every_inner_seam(oracle, name):
    """meshio.weld_lattice on the oracle's mesh of dense MPUs: the weld's contract holds, and no
    edge used by one triangle only lies inside the box (seams between MPUs are closed; the
    surface is open only where the box's faces cut it)."""
    om = du.oracle_mesh(oracle, name)
    model = du.model_of(name)
    assert not np.isnan(om.pos).any()
    mesh = meshio.TriMesh(om.pos, om.global_tris(), om.nrm, om.col)
    w, vmap = meshio.weld_lattice(mesh, om.vertex_offsets, du.CS, *model.bbox)
    check_contract(om.pos, om.nrm, om.col, om.global_tris(), w, vmap)
    assert w.n_vertices < len(om.pos) and w.n_triangles == len(om.tris)
    inner, total = du.interior_open_edges(w.tris, w.pos, soa.mpu_dims(du.CS, *model.bbox))
    assert inner == 0, (inner, total)
    assert total == meshio.open_edge_count(w.tris)
    # unwelded, the seams are open: the weld is what closes them
    assert du.interior_open_edges(om.global_tris(), om.pos, soa.mpu_dims(du.CS, *model.bbox))[0] > 0
