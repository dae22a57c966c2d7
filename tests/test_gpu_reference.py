"""The HIP path against the reference's own recorded output (tests/golden/reference/*.npz, written
by tests/golden/make_reference_goldens.py from the compiled PS::SIMDPOLY), not against the
oracle: C1 and eight trees without Disc / Ring / RicciBlend in cubes and three more in boxes whose
lattices are (8,5,3), (5,3,8) and (3,8,5), where every bit the reference
computes is plain IEEE arithmetic -- per-MPU ctFieldEvals / V / T, offsets, MPU-local
triangles, positions and colours bit-exact; normals within 2e-3 (the reference normalises with
rsqrtps); fieldValue and fieldValueAndColor at recorded points bit-exact.  Interpreter and
generated kernels, with and without k_front."""
import numpy as np
import pytest

import reference_util as ru
from parity_util import assert_bits_equal, assert_mesh_matches
from parsip_amd import gpu

pytestmark = pytest.mark.gpu

NORMALS_ATOL = 2e-3


@pytest.fixture(scope="module")
def recorded():
    return {n: ru.load_fixture(n) for n in ru.fixture_names()}


@pytest.mark.parametrize("jit", [0, 1])
@pytest.mark.parametrize("name", ru.fixture_names())
def test_mesh_equals_recorded_reference(gpu_poly, recorded, name, jit):
    model, cs, _, ref_mesh = recorded[name]
    try:
        gpu_poly.set_option(gpu.OPT_JIT, jit)
        gpu_poly.set_model(model)
        assert gpu_poly.jit_active == bool(jit)
        for front in (0, 2):
            gpu_poly.set_option(gpu.OPT_FRONT, front)
            info = gpu_poly.run(cs)
            assert (info.ctMPUs, info.ctVertices, info.ctTriangles) == \
                (len(ref_mesh.stats), len(ref_mesh.pos), len(ref_mesh.tris)), front
            assert_mesh_matches(gpu_poly.download(), gpu_poly.stats(), ref_mesh, normals_atol=NORMALS_ATOL)
    finally:  # the session's context goes back to the defaults
        gpu_poly.set_option(gpu.OPT_JIT, 1)
        gpu_poly.set_option(gpu.OPT_FRONT, 2)


@pytest.mark.parametrize("name", ru.fixture_names())
def test_field_probes_equal_recorded_reference(gpu_poly, recorded, name):
    model, _, d, _ = recorded[name]
    gpu_poly.set_model(model)
    q = d["quad_xyz"]
    assert_bits_equal(gpu_poly.field_values(q, mode=0), d["quad_field"], "fieldValue (4-lane groups)")
    f, c = gpu_poly.field_values(q[::4], mode=2)
    assert_bits_equal(f, d["point_field"], "fieldValueAndColor field")
    assert_bits_equal(c, d["point_colour"], "fieldValueAndColor colour")
    assert np.count_nonzero(d["quad_field"]) > 0
