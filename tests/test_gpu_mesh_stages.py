"""The branches of the shared mesh stages (parsip_amd/csrc/psgpu_mesh_stages.h; DESIGN.md §6
"Mesh stages") that the other weld, shells and filter tests reach only in part: the scalar
tails of the 16-byte loads for every residue of the element counts, a mesh smaller than one
wave, and k_weld_scan over more than 256 blocks.  tests/test_mesh_stages.py checks that the
inputs have those counts.  Polygonization is not under test: the runs use the interpreter."""
import numpy as np
import pytest

from parsip_amd import gpu, meshio
from weld_util import SCAN_COUNTS, SCAN_NAME, TAIL_COUNTS, make_case

pytestmark = pytest.mark.gpu

_RUNS = {}


@pytest.fixture(scope="module")
def poly():
    assert gpu.device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"
    p = gpu.Polygonizer(0)
    p.set_option(gpu.OPT_JIT, 0)
    yield p
    p.close()


def weld_bytes(w):
    return tuple(np.ascontiguousarray(a).tobytes() for a in (w.pos, w.nrm, w.col, w.tris, w.vertex_map))


def device_case(poly, name):
    """One run of a named input, computed once: (device weld, device shells, host weld, host
    map, [(mask, device filter)] for the all-zero filter and the case's mask: the even-indexed
    shells, or for the scan's input all but the largest)."""
    if name not in _RUNS:
        model, cs, (b, e) = make_case(name)
        poly.set_model(model)
        poly.run(cs, b, e)
        mesh = poly.download()
        w = poly.weld()
        sh = poly.weld_shells()
        mask = (np.arange(len(sh.shells)) % 2 == 0).astype(np.uint8)
        if name == SCAN_NAME:
            mask[:] = 1
            mask[int(np.argmax(sh.shells["ctVertices"]))] = 0
        filters = [(m, poly.weld_filter(None, m)) for m in (None, mask)]
        ref, ref_map = meshio.weld_lattice(mesh, mesh.vertex_offsets, cs, *model.bbox, mpu_begin=b)
        _RUNS[name] = (w, sh, ref, ref_map, filters)
    return _RUNS[name]


def assert_host_forms(w, sh, ref, ref_map, filters):
    """Weld, shells and both filters, byte for byte."""
    assert (len(w.pos), len(w.tris)) == (w.info.ctVertices, w.info.ctTriangles) == (ref.n_vertices, ref.n_triangles)
    for what, got, want in (("pos", w.pos, ref.pos), ("nrm", w.nrm, ref.nrm), ("col", w.col, ref.col)):
        assert got.tobytes() == np.ascontiguousarray(want, np.float32).tobytes(), what
    assert np.array_equal(w.tris, ref.tris.astype(np.uint32))
    assert np.array_equal(w.vertex_map, ref_map.astype(np.uint32))
    assert sh.tobytes() == meshio.shells(w.pos, w.tris).tobytes()
    for mask, got in filters:
        want = meshio.filter_shells(w.pos, w.nrm, w.col, w.tris, sh, None, mask)
        for a in ("pos", "nrm", "col", "tris", "vertex_map", "shell_map"):
            assert getattr(got, a).tobytes() == getattr(want, a).tobytes(), a
        assert got.tobytes() == want.tobytes()
    every = filters[0][1]
    assert (every.pos.tobytes(), every.tris.tobytes()) == (w.pos.tobytes(), w.tris.tobytes())


def group_weld(name, bounds):
    """The weld, shells and all-zero filter of a 2-part group split at `bounds` (None: planned)."""
    model, cs, _ = make_case(name)
    g = gpu.Group([0, 0])
    try:
        g.set_option(gpu.OPT_JIT, 0)
        g.set_model(model)
        if bounds:
            g.set_split(bounds)
        g.run(cs)
        return g.weld(), g.weld_shells(), g.weld_filter()
    finally:
        g.close()


@pytest.mark.parametrize("name", list(TAIL_COUNTS))
def test_tails_equal_the_host_forms(poly, name):
    w, sh, ref, ref_map, filters = device_case(poly, name)
    assert (w.info.ctInputVertices, w.info.ctTriangles, w.info.ctVertices) == TAIL_COUNTS[name]
    assert_host_forms(w, sh, ref, ref_map, filters)
    mask, kept = filters[1]
    assert len(kept.shells) == int(mask.sum()) and len(kept.pos) == int(sh.shells["ctVertices"][mask != 0].sum())


@pytest.mark.parametrize("name", ["rand1_0.13_mpus_0_54", "rand1_0.13_mpus_0_85"])
def test_tails_in_a_group(poly, name):
    w, sh, _, _, filters = device_case(poly, name)
    end = int(name.rsplit("_", 1)[1])
    gw, gsh, gf = group_weld(name, [0, end // 2, end])
    assert gw.info.ctInputVertices == TAIL_COUNTS[name][0]
    assert weld_bytes(gw) == weld_bytes(w)
    assert gsh.tobytes() == sh.tobytes() and gf.tobytes() == filters[0][1].tobytes()


def test_scan_over_more_than_256_blocks(poly):
    """495, 381 and 759 block counts through k_weld_scan's carry loop."""
    w, sh, ref, ref_map, filters = device_case(poly, SCAN_NAME)
    assert (w.info.ctInputVertices, w.info.ctTriangles, w.info.ctVertices) == SCAN_COUNTS[1:]
    assert_host_forms(w, sh, ref, ref_map, filters)
    kept = filters[1][1]
    assert 256 * 256 < len(kept.tris) < len(w.tris) and 0 < len(kept.pos) < len(w.pos)


def test_scan_in_a_group(poly):
    w = device_case(poly, SCAN_NAME)[0]
    gw, _, _ = group_weld(SCAN_NAME, None)
    assert gw.info.ctInputVertices == SCAN_COUNTS[1]
    assert weld_bytes(gw) == weld_bytes(w)
