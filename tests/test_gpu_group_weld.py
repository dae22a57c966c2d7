"""The weld of a group's parts into one watertight mesh (psgpu_group_weld,
parsip_amd/csrc/psgpu_group.cpp and psgpu_weld.hip; DESIGN.md §6 "Weld of a group"): byte for
byte the single context's weld of the whole lattice for any number of parts and any split,
the host definition (meshio.weld_lattice on the group's download), and the C-ABI's rules
around it.  The parts share device 0, as in tests/test_gpu_multi.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import dense_util as du
from parsip_amd import gpu, meshio, soa, synth
from weld_util import check_contract, golden_counts, make_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["C1", "rand3_0.071", "rand1_0.13", "C2"]
_SINGLE = {}
_GROUPS = {}


def weld_bytes(w):
    return tuple(np.ascontiguousarray(a).tobytes() for a in (w.pos, w.nrm, w.col, w.tris, w.vertex_map))


def counts(info):
    return (info.ctVertices, info.ctTriangles, info.ctInputVertices, info.ctSeamVertices)


def mesh_bytes(m):
    return tuple(np.ascontiguousarray(a).tobytes() for a in (m.pos, m.nrm, m.col, m.tris, m.vertex_offsets,
                                                             m.triangle_offsets))


@pytest.fixture(scope="module")
def single():
    """name -> Polygonizer.weld() of the full-range run on one context (computed once, shared)."""
    assert gpu.device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"
    p = gpu.Polygonizer(0)

    def get(name):
        if name not in _SINGLE:
            model, cs, _ = make_case(name)
            p.set_model(model)
            p.run(cs)
            _SINGLE[name] = p.weld()
        return _SINGLE[name]

    yield get
    p.close()


@pytest.fixture(scope="module")
def groups():
    """k -> a Group of k parts on device 0 with default options (tests that change options or
    the split make their own)."""
    def get(k):
        if k not in _GROUPS:
            _GROUPS[k] = gpu.Group([0] * k)
        return _GROUPS[k]

    yield get
    for g in _GROUPS.values():
        g.close()
    _GROUPS.clear()


def group_run(g, name):
    model, cs, _ = make_case(name)
    g.set_model(model)
    return model, cs, g.run(cs)


def ctx_weld(ptr):
    """psgpu_weld + psgpu_download_weld on a bare context pointer (a group's part)."""
    L = gpu.load()
    c = ctypes.c_void_p(ptr)
    info = gpu.PsWeldInfo()
    assert L.psgpu_weld(c, ctypes.byref(info)) == soa.RET_SUCCESS
    pos = np.zeros((info.ctVertices, 3), np.float32)
    tris = np.zeros((info.ctTriangles, 3), np.uint32)
    assert L.psgpu_download_weld(c, pos.ctypes.data, None, None, tris.ctypes.data, None) == soa.RET_SUCCESS
    return info, pos, tris


# ---- equals the single context ------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 8])
@pytest.mark.parametrize("name", CASES)
def test_group_weld_equals_single_context(single, groups, name, k):
    """The default (planned) split into k parts: pos, nrm, col, tris, vertex_map and the four
    counts of Group.weld() equal Polygonizer.weld() of the full-range run."""
    want = single(name)
    g = groups(k)
    _, _, (total, parts) = group_run(g, name)
    w = g.weld()
    assert counts(w.info) == counts(want.info)
    assert w.info.ctInputVertices == total.ctVertices and w.info.ctTriangles == total.ctTriangles
    assert weld_bytes(w) == weld_bytes(want)


# ---- fixed splits that cut everywhere -----------------------------------------------------
@pytest.mark.parametrize("bounds", [[0, 100, 100, 250, 500, 729], [0, 243, 486, 729]])
def test_group_weld_fixed_splits(single, bounds):
    """rand3 at 0.071 (9^3 MPUs) with an empty part, a bound inside a z-row of 9 and one inside
    a slab of 81; and in thirds along x.  The same bytes as one context, watertight, 3,334
    vertices.  The middle third welded alone through its context leaves 74 open edges (the
    golden of MPUs [243, 486)): the group weld closes those seams."""
    want = single("rand3_0.071")
    g = gpu.Group([0] * (len(bounds) - 1))
    try:
        g.set_split(bounds)
        _, _, (total, parts) = group_run(g, "rand3_0.071")
        assert [(p.mpuBegin, p.mpuEnd) for p in parts] == list(zip(bounds[:-1], bounds[1:]))
        w = g.weld()
        assert weld_bytes(w) == weld_bytes(want) and counts(w.info) == counts(want.info)
        assert meshio.open_edge_count(w.tris) == 0 and w.info.ctVertices == 3334
        if bounds == [0, 243, 486, 729]:
            gold = golden_counts()["rand3_0.071_mpus_243_486"]["lattice_weld"]
            assert (gold["vertices"], gold["open_edges"]) == (2530, 74)
            info, _, tris = ctx_weld(g.context_ptr(1))
            assert (info.ctVertices, meshio.open_edge_count(tris)) == (2530, 74)
            assert weld_bytes(g.weld()) == weld_bytes(want)  # the part's own weld disturbs nothing
    finally:
        g.close()


# ---- equals the host definition -----------------------------------------------------------
def test_group_weld_equals_host_definition(groups):
    g = groups(3)
    model, cs, _ = group_run(g, "rand3_0.071")
    mesh = g.download()
    w = g.weld()
    ref, ref_map = meshio.weld_lattice(mesh, mesh.vertex_offsets, cs, *model.bbox)
    assert (len(w.pos), len(w.tris)) == (ref.n_vertices, ref.n_triangles)
    for what, got, exp in (("pos", w.pos, ref.pos), ("nrm", w.nrm, ref.nrm), ("col", w.col, ref.col)):
        assert got.tobytes() == np.ascontiguousarray(exp, np.float32).tobytes(), what
    assert np.array_equal(w.tris, ref.tris.astype(np.uint32))
    assert np.array_equal(w.vertex_map, ref_map.astype(np.uint32))
    check_contract(mesh.pos, mesh.nrm, mesh.col, mesh.tris, w, w.vertex_map)


# ---- other behaviour ----------------------------------------------------------------------
def test_group_weld_on_another_part_and_twice(single, groups):
    want = weld_bytes(single("rand3_0.071"))
    g = groups(3)
    group_run(g, "rand3_0.071")
    assert weld_bytes(g.weld(0)) == want
    d = g.weld_device()
    assert all(getattr(d, f) for f in ("pos", "nrm", "col", "tris", "vertexMap"))
    assert weld_bytes(g.weld(0)) == want      # twice
    assert weld_bytes(g.weld(2)) == want      # the buffers move to part 2's
    assert all(getattr(g.weld_device(), f) for f in ("pos", "nrm", "col", "tris", "vertexMap"))
    assert weld_bytes(g.weld(1)) == want


def test_group_weld_after_reruns_for_capacity(single):
    """Capacity 64 before the first run: every part's finish re-runs its range with grown
    buffers, and records, offsets and counters are the final runs'."""
    want = weld_bytes(single("rand3_0.071"))
    g = gpu.Group([0] * 3)
    try:
        g.set_option(gpu.OPT_CAPACITY, 64)
        _, _, (total, parts) = group_run(g, "rand3_0.071")
        assert total.launchFlags & gpu.LAUNCH_RERUN
        assert weld_bytes(g.weld()) == want
    finally:
        g.close()


def test_group_weld_leaves_the_run_as_it_found_it(groups):
    """run -> weld -> run: the group's download is the same bytes before the weld, after it and
    after the second run."""
    g = groups(3)
    _, cs, _ = group_run(g, "rand1_0.13")
    first = mesh_bytes(g.download())
    g.weld()
    assert mesh_bytes(g.download()) == first
    g.run(cs)
    assert mesh_bytes(g.download()) == first


def test_group_weld_of_an_empty_mesh(groups):
    model, cs, _ = synth.make_config("C1")
    model.prims["bboxLo"][0] = (5.0, 5.0, 5.0)
    model.prims["bboxHi"][0] = (6.0, 6.0, 6.0)
    g = groups(2)
    g.set_model(model)
    total, _ = g.run(cs)
    assert total.ctMPUs > 0 and (total.ctVertices, total.ctTriangles) == (0, 0)
    w = g.weld()
    assert counts(w.info) == (0, 0, 0, 0)
    assert len(w.pos) == len(w.tris) == len(w.vertex_map) == 0
    g.weld_device()


def test_group_weld_times(single):
    """With OPT_KERNEL_TIMING on the group: eight phases, the whole weld first, and the phases
    after it add up to it (they are consecutive intervals on one stream)."""
    g = gpu.Group([0] * 2)
    try:
        g.set_option(gpu.OPT_KERNEL_TIMING, 1)
        group_run(g, "rand3_0.071")
        assert weld_bytes(g.weld()) == weld_bytes(single("rand3_0.071"))
        t = g.weld_times()
        ms = list(t.values())
        assert len(t) == 8 and list(t)[0] == "group weld total" and ms[0] > 0 and min(ms) >= 0
        assert abs(sum(ms[1:]) - ms[0]) < 1e-3 + 1e-3 * ms[0]  # hipEvent differences of one stream
    finally:
        g.close()


# ---- errors -------------------------------------------------------------------------------
def no_weld(L, g):
    d = gpu.PsWeldDevice()
    return (L.psgpu_group_weld_device(g._g, ctypes.byref(d)),
            L.psgpu_group_download_weld(g._g, None, None, None, None, None)) == (soa.RET_PARAM_ERROR,) * 2


def test_group_weld_errors():
    L = gpu.load()
    info = gpu.PsWeldInfo()
    g = gpu.Group([0] * 3)
    try:
        weld = lambda part=0: L.psgpu_group_weld(g._g, part, ctypes.byref(info))  # noqa: E731
        assert weld() == soa.RET_PARAM_ERROR and no_weld(L, g)                     # no run, no model
        model, cs, _ = make_case("C1")
        g.set_model(model)
        assert weld() == soa.RET_PARAM_ERROR and no_weld(L, g)                     # a model, no run
        g.run(cs)
        assert no_weld(L, g)                                                       # a run, no weld
        with pytest.raises(gpu.PsgpuError):
            g.weld_device()
        assert weld(-1) == soa.RET_PARAM_ERROR and weld(3) == soa.RET_PARAM_ERROR  # dstPart out of range
        assert no_weld(L, g)
        assert g.weld().info.ctVertices == 1014 and not no_weld(L, g)
        g.set_model(model)                                                         # supersedes the run
        assert no_weld(L, g) and weld() == soa.RET_PARAM_ERROR
        g.run(cs)
        assert no_weld(L, g)                                                       # the weld was of the old run
        assert g.weld().info.ctVertices == 1014 and not no_weld(L, g)
        g.polygonize(cs)
        g.finish()
        assert no_weld(L, g)
        assert g.weld().info.ctVertices == 1014 and not no_weld(L, g)
        g.set_split([0, 40, 80, 125])
        assert no_weld(L, g)
        g.run(cs)
        assert g.weld().info.ctVertices == 1014 and not no_weld(L, g)
        g.set_option(gpu.OPT_CAPACITY, 1 << 20)                                    # the parts drop their runs
        assert no_weld(L, g) and weld() == soa.RET_PARAM_ERROR
        g.run(cs)
        assert g.weld().info.ctVertices == 1014
    finally:
        g.close()


def test_group_weld_refuses_a_superseded_part():
    """A run made through a part's own context pointer after the group's finish: that part no
    longer holds the range the group collected, so the group's weld is refused until the group
    runs again."""
    L = gpu.load()
    info = gpu.PsWeldInfo()
    g = gpu.Group([0] * 3)
    try:
        model, cs, _ = make_case("C1")
        g.set_model(model)
        _, parts = g.run(cs)
        assert g.weld().info.ctVertices == 1014
        c = ctypes.c_void_p(g.context_ptr(1))
        assert L.psgpu_polygonize(c, cs, parts[1].mpuBegin, parts[1].mpuEnd, None) == soa.RET_SUCCESS
        assert L.psgpu_group_weld(g._g, 0, ctypes.byref(info)) == soa.RET_PARAM_ERROR  # pending on the part
        assert L.psgpu_finish(c, ctypes.byref(gpu.PsMeshInfo())) == soa.RET_SUCCESS
        assert L.psgpu_group_weld(g._g, 0, ctypes.byref(info)) == soa.RET_PARAM_ERROR  # finished, not the group's
        g.run(cs)
        assert g.weld().info.ctVertices == 1014
    finally:
        g.close()


def test_group_weld_refuses_an_overflow_run():
    """dense_util's `mixed` (8 MPUs, 4 and 7 past 512 triangles): the group's run succeeds and
    reports MPU 4, its weld is refused."""
    L = gpu.load()
    g = gpu.Group([0] * 2)
    try:
        g.set_option(gpu.OPT_JIT, 0)
        g.set_split([0, 3, 8])
        g.set_model(du.model_of("mixed"))
        total, _ = g.run(du.CS)
        assert total.firstOverflowMPU == 4 and total.ctVertices > 0
        assert L.psgpu_group_weld(g._g, 0, ctypes.byref(gpu.PsWeldInfo())) == soa.RET_PARAM_ERROR
        assert no_weld(L, g)
    finally:
        g.close()


# ---- the C++ face -------------------------------------------------------------------------
def test_cpp_simdpolyt_weld(single, tmp_path):
    """psgpu::SimdPolyT::weld() compiled as a host would compile it (tests/cpp/group_weld_check.cpp,
    over the mock BlobTree) on C1 as two parts: PARAM_ERROR before run(), then 1,014 vertices /
    2,024 triangles and the same bytes as Polygonizer.weld() of C1."""
    from parsip_amd import blobtree as bt
    from test_cpp_simdpoly import write_tree

    gpp = shutil.which("g++")
    assert gpp is not None, "g++ is needed to compile the C++ face"
    lib_dir = os.path.join(ROOT, "parsip_amd")
    exe = tmp_path / "group_weld_check"
    subprocess.run([gpp, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "group_weld_check.cpp"),
                    "-L", lib_dir, "-l:libparsip_gpu.so", f"-Wl,-rpath,{lib_dir}", "-o", str(exe)], check=True)
    c1, cs, _ = make_case("C1")
    # C1 as a BlobTree: one Point at the origin in C1's colour, its octree C1's scene box
    root = bt.Point((0.0, 0.0, 0.0), material=bt.Material(diffused=(0.0, 0.0, 0.0, 1.0)))
    root.octree = (np.array(c1.bbox[0], np.float32), np.array(c1.bbox[1], np.float32))
    tree, out = tmp_path / "tree.txt", tmp_path / "weld.bin"
    write_tree(root, str(tree))
    r = subprocess.run([str(exe), str(tree), repr(float(cs)), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    rc = np.frombuffer(raw[:16], np.int32)
    assert rc[0] == soa.RET_PARAM_ERROR and (rc[1:] == soa.RET_SUCCESS).all()
    vw, t, vin, seam, run_v, run_t, n_parts, split = (int(x) for x in np.frombuffer(raw[16:48], np.uint32))
    assert n_parts == 2 and 0 < split < 125                       # C1 really ran as two parts
    assert (vw, t) == (1014, 2024) and (vin, run_v, run_t) == (1326, 1326, 2024) and 0 < seam < vin
    want = single("C1")
    assert seam == want.info.ctSeamVertices
    assert raw[48:] == b"".join(weld_bytes(want))
