"""The device weld (psgpu_weld, parsip_amd/csrc/psgpu_weld.hip; DESIGN.md §6 "Weld"): the
finished run's mesh welded by lattice-edge identity, byte for byte against
meshio.weld_lattice applied to the same run's download, and the C-ABI's rules around it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from parity_util import mesh_digests
from parsip_amd import gpu, meshio, soa, synth
from weld_util import check_contract, golden_counts, make_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_CASES = ["C1", "rand3_0.071", "rand1_0.13", "C2", "rand3_0.071_mpus_243_486"]
_RUNS = {}


@pytest.fixture(scope="module")
def poly():
    """A context of this module's own (the tests below change its options)."""
    assert gpu.device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"
    p = gpu.Polygonizer(0)
    yield p
    p.close()


def weld_bytes(w):
    return tuple(np.ascontiguousarray(a).tobytes() for a in (w.pos, w.nrm, w.col, w.tris, w.vertex_map))


def run_and_weld(p, name):
    model, cs, (b, e) = make_case(name)
    p.set_model(model)
    info = p.run(cs, b, e)
    return model, cs, b, info, p.download(), p.weld()


def device_case(poly, name):
    """One run of a named input on the module's context with default options: (model,
    cellsize, mpu_begin, run info, download, device weld, host reference weld + map)."""
    if name not in _RUNS:
        model, cs, b, info, mesh, w = run_and_weld(poly, name)
        ref, ref_map = meshio.weld_lattice(mesh, mesh.vertex_offsets, cs, *model.bbox, mpu_begin=b)
        _RUNS[name] = (model, cs, b, info, mesh, w, ref, ref_map)
    return _RUNS[name]


@pytest.mark.parametrize("name", PARITY_CASES)
def test_weld_equals_host_reference(poly, name):
    """pos, nrm, col, tris and vertex_map of Polygonizer.weld() are byte-equal to
    meshio.weld_lattice on the same run's download() (full ranges and MPUs [243, 486))."""
    _, _, _, info, mesh, w, ref, ref_map = device_case(poly, name)
    assert w.info.ctInputVertices == info.ctVertices == len(mesh.pos) > 0
    assert (len(w.pos), len(w.tris)) == (w.info.ctVertices, w.info.ctTriangles) == (ref.n_vertices, ref.n_triangles)
    for what, got, want in (("pos", w.pos, ref.pos), ("nrm", w.nrm, ref.nrm), ("col", w.col, ref.col)):
        assert got.tobytes() == np.ascontiguousarray(want, np.float32).tobytes(), what
    assert np.array_equal(w.tris, ref.tris.astype(np.uint32))
    assert np.array_equal(w.vertex_map, ref_map.astype(np.uint32))
    check_contract(mesh.pos, mesh.nrm, mesh.col, mesh.tris, w, w.vertex_map)


@pytest.mark.parametrize("name", PARITY_CASES)
def test_weld_counts_match_golden(poly, name):
    gold = golden_counts()[name]
    model, cs, b, info, mesh, w, _, _ = device_case(poly, name)
    assert (w.info.ctInputVertices, w.info.ctTriangles) == (gold["vertices"], gold["triangles"])
    assert w.info.ctTriangles == info.ctTriangles
    assert w.info.ctVertices == gold["lattice_weld"]["vertices"]
    assert meshio.open_edge_count(w.tris) == gold["lattice_weld"]["open_edges"]
    # input vertices on an MPU face: an off-axis lattice coordinate on a multiple of 7
    g = meshio.lattice_edges(mesh, mesh.vertex_offsets, cs, *model.bbox, mpu_begin=b)
    off_axis = np.arange(3)[None, :] != g[:, 3:4]
    assert w.info.ctSeamVertices == int(((g[:, :3] % 7 == 0) & off_axis).any(axis=1).sum())


def test_weld_is_watertight_where_the_bit_weld_is_not(poly):
    """rand3 at cell size 0.071: a closed surface inside the box.  The device returns a mesh
    with no open edge; meshio.weld on the same download leaves 1,276."""
    _, _, _, _, mesh, w, _, _ = device_case(poly, "rand3_0.071")
    assert meshio.open_edge_count(w.tris) == 0
    assert w.info.ctVertices == 3334
    wb = meshio.weld(meshio.from_mesh(mesh))
    assert (wb.n_vertices, meshio.open_edge_count(wb.tris)) == (3998, 1276)


def test_weld_after_a_rerun_for_capacity(poly):
    """A finish that re-ran the polygonization with grown buffers (capacity 64 before the
    first run) leaves records, offsets and counters of the final run: the same weld."""
    want = weld_bytes(device_case(poly, "rand3_0.071")[5])
    p = gpu.Polygonizer(0)
    try:
        p.set_option(gpu.OPT_CAPACITY, 64)
        _, _, _, info, _, w = run_and_weld(p, "rand3_0.071")
        assert info.launchFlags & gpu.LAUNCH_RERUN
        assert weld_bytes(w) == want
    finally:
        p.close()


@pytest.mark.parametrize("front", [0, 1])
def test_weld_both_front_paths(poly, front):
    want = weld_bytes(device_case(poly, "rand3_0.071")[5])
    poly.set_option(gpu.OPT_FRONT, front)
    try:
        _, _, _, info, _, w = run_and_weld(poly, "rand3_0.071")
        assert bool(info.launchFlags & gpu.LAUNCH_FRONT) == bool(front)
        assert weld_bytes(w) == want
    finally:
        poly.set_option(gpu.OPT_FRONT, 2)


@pytest.mark.parametrize("jit", [0, 1])
def test_weld_both_jit_modes(poly, jit):
    want = weld_bytes(device_case(poly, "rand3_0.071")[5])
    poly.set_option(gpu.OPT_JIT, jit)
    try:
        _, _, _, _, _, w = run_and_weld(poly, "rand3_0.071")
        assert poly.jit_active == bool(jit)
        assert weld_bytes(w) == want
    finally:
        poly.set_option(gpu.OPT_JIT, 1)


def test_weld_twice_gives_the_same_bytes(poly):
    model, cs, _ = make_case("C2")
    poly.set_model(model)
    poly.run(cs)
    a = poly.weld()
    d1 = poly.weld_device()
    b = poly.weld()
    assert weld_bytes(a) == weld_bytes(b) == weld_bytes(device_case(poly, "C2")[5])
    assert all(getattr(d1, f) for f in ("pos", "nrm", "col", "tris", "vertexMap"))


def test_weld_leaves_the_context_as_it_found_it(poly):
    """run -> weld -> run: the second run's mesh digests equal the first's, and the first
    run's own buffers still download the same mesh after the weld."""
    model, cs, _ = make_case("rand1_0.13")
    poly.set_model(model)

    def digests():
        gm, gs = poly.download(), poly.stats()
        st = np.stack([gs["passedPrecheck"], gs["ctFieldEvals"], gs["ctVertices"], gs["ctTriangles"]], axis=1)
        return mesh_digests(st, gm.pos, gm.nrm, gm.col, gm.local_tris())

    poly.run(cs)
    first = digests()
    poly.weld()
    assert digests() == first
    poly.run(cs)
    assert digests() == first


def test_weld_errors(poly):
    L = gpu.load()
    p = gpu.Polygonizer(0)
    try:
        info = gpu.PsWeldInfo()
        assert L.psgpu_weld(p._ctx, info) == soa.RET_PARAM_ERROR                       # no run yet
        model, cs, _ = make_case("C1")
        p.set_model(model)
        assert L.psgpu_weld(p._ctx, info) == soa.RET_PARAM_ERROR                       # a model, no run
        p.polygonize(cs)
        assert L.psgpu_weld(p._ctx, info) == soa.RET_PARAM_ERROR                       # not finished
        p.finish()
        d = gpu.PsWeldDevice()
        assert L.psgpu_weld_device(p._ctx, d) == soa.RET_PARAM_ERROR                   # no weld yet
        assert L.psgpu_download_weld(p._ctx, None, None, None, None, None) == soa.RET_PARAM_ERROR
        with pytest.raises(gpu.PsgpuError):
            p.weld_device()
        assert p.weld().info.ctVertices == 1014
        assert L.psgpu_weld_device(p._ctx, d) == soa.RET_SUCCESS
        p.set_model(model)                                                             # supersedes the run
        assert L.psgpu_weld(p._ctx, info) == soa.RET_PARAM_ERROR
        assert L.psgpu_weld_device(p._ctx, d) == soa.RET_PARAM_ERROR
        p.polygonize(cs)
        assert L.psgpu_download_weld(p._ctx, None, None, None, None, None) == soa.RET_PARAM_ERROR
        p.finish()
        assert L.psgpu_weld_device(p._ctx, d) == soa.RET_PARAM_ERROR                   # the weld was of the old run
        assert p.weld().info.ctVertices == 1014
    finally:
        p.close()


def test_weld_of_an_empty_mesh(poly):
    """A model whose surface lies outside the box: 0 vertices, 0 triangles, success."""
    model, cs, _ = synth.make_config("C1")
    model.prims["bboxLo"][0] = (5.0, 5.0, 5.0)
    model.prims["bboxHi"][0] = (6.0, 6.0, 6.0)
    poly.set_model(model)
    info = poly.run(cs)
    assert info.ctMPUs > 0 and (info.ctVertices, info.ctTriangles) == (0, 0)
    w = poly.weld()
    assert (w.info.ctVertices, w.info.ctTriangles, w.info.ctInputVertices, w.info.ctSeamVertices) == (0, 0, 0, 0)
    assert len(w.pos) == len(w.tris) == len(w.vertex_map) == 0
    poly.weld_device()


def test_cpp_simdpoly_weld(poly, tmp_path):
    """psgpu::SimdPolyGpu::weld() compiled as a host would compile it (tests/cpp/weld_check.cpp)
    on C1: PARAM_ERROR before a run, then 1,014 vertices / 2,024 triangles and the same bytes
    as Polygonizer.weld()."""
    gpp = shutil.which("g++")
    assert gpp is not None, "g++ is needed to compile the C++ face"
    lib_dir = os.path.join(ROOT, "parsip_amd")
    exe = tmp_path / "weld_check"
    subprocess.run([gpp, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "weld_check.cpp"), "-L", lib_dir, "-l:libparsip_gpu.so",
                    f"-Wl,-rpath,{lib_dir}", "-o", str(exe)], check=True)
    model, cs, _ = make_case("C1")
    src, out = tmp_path / "soa.bin", tmp_path / "weld.bin"
    with open(src, "wb") as f:
        f.write(model.prims.tobytes() + model.mats.tobytes() + model.ops.tobytes())
    r = subprocess.run([str(exe), str(src), repr(float(cs)), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    rc = np.frombuffer(raw[:20], np.int32)
    assert rc[0] == soa.RET_PARAM_ERROR and (rc[1:] == soa.RET_SUCCESS).all()
    vw, t, vin, seam, run_v, run_t = (int(x) for x in np.frombuffer(raw[20:44], np.uint32))
    assert (vw, t) == (1014, 2024) and (vin, run_v, run_t) == (1326, 1326, 2024) and 0 < seam < vin
    want = device_case(poly, "C1")[5]
    assert raw[44:] == b"".join(weld_bytes(want))
