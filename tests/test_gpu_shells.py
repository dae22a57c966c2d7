"""The shells of the device weld (psgpu_weld_shells / psgpu_group_weld_shells,
parsip_amd/csrc/psgpu_shells.hip; DESIGN.md §6 "Shells"): byte for byte meshio.shells of the
weld's own download, the committed counts, the same bytes twice, a group against a context,
and the C-ABI's rules around the calls."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from parity_util import mesh_digests
from parsip_amd import gpu, meshio, soa, synth
from shells_util import counts, golden_counts, integer_counts, make_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what each case exercises: C1 one shell over several blocks (waves and blocks that agree);
# rand4 two closed shells; rand1 two interleaved open shells (mixed waves); the sub-range seams
# left open; C2 ~100 blocks, 75 k edges in the table and a 6-vertex shell; the non-manifold
# edge; the cavity
CASES = ["C1", "rand4_0.123457", "rand1_0.13", "rand3_0.071_mpus_243_486", "C2", "ring_union_point",
         "cube_minus_point"]
_RUNS = {}


@pytest.fixture(scope="module")
def poly():
    assert gpu.device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"
    p = gpu.Polygonizer(0)
    yield p
    p.close()


def weld_bytes(w):
    return tuple(np.ascontiguousarray(a).tobytes() for a in (w.pos, w.nrm, w.col, w.tris, w.vertex_map))


def run_weld(p, name):
    model, cs, (b, e) = make_case(name)
    p.set_model(model)
    p.run(cs, b, e)
    return p.weld()


def device_case(poly, name):
    """(device weld, device shells, meshio.shells of that weld's download), computed once."""
    if name not in _RUNS:
        w = run_weld(poly, name)
        sh = poly.weld_shells()
        _RUNS[name] = (w, sh, meshio.shells(w.pos, w.tris))
    return _RUNS[name]


def assert_same(got, want):
    """Field by field first (a readable failure), then every byte."""
    assert got.info["ctShells"] == want.info["ctShells"] == len(got.shells)
    for f in meshio.SHELL_DTYPE.names:
        assert got.shells[f].tobytes() == want.shells[f].tobytes(), (f, got.shells[f], want.shells[f])
    for f in meshio.SHELLS_INFO_DTYPE.names:
        assert got.info[f].tobytes() == want.info[f].tobytes(), (f, got.info[f], want.info[f])
    assert np.array_equal(got.vertex_shell, want.vertex_shell) and np.array_equal(got.tri_shell, want.tri_shell)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", CASES)
def test_shells_equal_host_form(poly, name):
    w, sh, ref = device_case(poly, name)
    assert (sh.info["ctVertices"], sh.info["ctTriangles"]) == (w.info.ctVertices, w.info.ctTriangles)
    assert len(sh.vertex_shell) == len(w.pos) and len(sh.tri_shell) == len(w.tris)
    assert_same(sh, ref)


@pytest.mark.parametrize("name", CASES)
def test_shells_counts_match_golden(poly, name):
    _, sh, _ = device_case(poly, name)
    assert integer_counts(counts(sh)) == integer_counts(golden_counts()[name])


def test_shells_twice_give_the_same_bytes_and_disturb_nothing(poly):
    """Two calls on one weld: equal bytes; the weld's download and the run's mesh digests are
    what they were before the calls; the device pointers are set."""
    model, cs, _ = make_case("rand1_0.13")
    poly.set_model(model)
    poly.run(cs)

    def digests():
        gm, gs = poly.download(), poly.stats()
        st = np.stack([gs["passedPrecheck"], gs["ctFieldEvals"], gs["ctVertices"], gs["ctTriangles"]], axis=1)
        return mesh_digests(st, gm.pos, gm.nrm, gm.col, gm.local_tris())

    first = digests()
    w = poly.weld()
    a = poly.weld_shells()
    d = poly.weld_shells_device()
    b = poly.weld_shells()
    assert a.tobytes() == b.tobytes() == device_case(poly, "rand1_0.13")[1].tobytes()
    assert d.shells and d.vertexShell and d.triShell
    L = gpu.load()
    pos, tris = np.zeros_like(w.pos), np.zeros_like(w.tris)
    nrm, col, vmap = np.zeros_like(w.nrm), np.zeros_like(w.col), np.zeros_like(w.vertex_map)
    assert L.psgpu_download_weld(poly._ctx, pos.ctypes.data, nrm.ctypes.data, col.ctypes.data, tris.ctypes.data,
                                 vmap.ctypes.data) == soa.RET_SUCCESS
    assert weld_bytes(gpu.WeldedMesh(pos, nrm, col, tris, vmap, w.info)) == weld_bytes(w)
    assert digests() == first
    times = poly.weld_shells_times()
    assert len(times) == 11 and list(times)[0] == "shells total"


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("name", ["rand3_0.071", "rand1_0.13"])
def test_group_shells_equal_the_contexts(poly, name, k):
    want = device_case(poly, name)[1]
    model, cs, _ = make_case(name)
    g = gpu.Group([0] * k)
    try:
        g.set_model(model)
        g.run(cs)
        g.weld()
        sh = g.weld_shells()
        assert_same(sh, want)
        d = g.weld_shells_device()
        assert d.shells and d.vertexShell and d.triShell
        assert g.weld_shells().tobytes() == sh.tobytes()
    finally:
        g.close()


def test_shells_of_an_empty_mesh(poly):
    """A model whose surface lies outside the box: 0 shells and success, on a context and a group."""
    model, cs, _ = synth.make_config("C1")
    model.prims["bboxLo"][0] = (5.0, 5.0, 5.0)
    model.prims["bboxHi"][0] = (6.0, 6.0, 6.0)
    poly.set_model(model)
    poly.run(cs)
    assert poly.weld().info.ctVertices == 0
    sh = poly.weld_shells()
    assert sh.info.tobytes() == bytes(80) and len(sh.shells) == len(sh.vertex_shell) == len(sh.tri_shell) == 0
    assert sh.tobytes() == meshio.shells(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32)).tobytes()
    poly.weld_shells_device()
    g = gpu.Group([0] * 2)
    try:
        g.set_model(model)
        g.run(cs)
        g.weld()
        assert g.weld_shells().info.tobytes() == bytes(80)
    finally:
        g.close()


def no_shells(L, ctx, prefix="psgpu_"):
    d = gpu.PsShellsDevice()
    return (getattr(L, prefix + "weld_shells_device")(ctx, ctypes.byref(d)),
            getattr(L, prefix + "download_weld_shells")(ctx, None, 0, None, None)) == (soa.RET_PARAM_ERROR,) * 2


def test_shells_call_rules():
    L = gpu.load()
    p = gpu.Polygonizer(0)
    try:
        info = gpu.PsShellsInfo()
        shells = lambda: L.psgpu_weld_shells(p._ctx, ctypes.byref(info))  # noqa: E731
        assert shells() == soa.RET_PARAM_ERROR and no_shells(L, p._ctx)                 # no run yet
        model, cs, _ = make_case("rand4_0.123457")
        p.set_model(model)
        p.run(cs)
        assert shells() == soa.RET_PARAM_ERROR and no_shells(L, p._ctx)                 # a run, no weld
        p.weld()
        assert no_shells(L, p._ctx)                                                     # a weld, no shells call
        with pytest.raises(gpu.PsgpuError):
            p.weld_shells_device()
        assert shells() == soa.RET_SUCCESS and info.ctShells == 2 and not no_shells(L, p._ctx)
        assert L.psgpu_weld_shells(p._ctx, None) == soa.RET_SUCCESS                     # info may be NULL
        buf = np.zeros(2, meshio.SHELL_DTYPE)
        assert L.psgpu_download_weld_shells(p._ctx, buf.ctypes.data, 1, None, None) == soa.RET_PARAM_ERROR  # short
        assert L.psgpu_download_weld_shells(p._ctx, buf.ctypes.data, 2, None, None) == soa.RET_SUCCESS
        assert buf["firstVertex"].tolist() == [0, 403]
        assert L.psgpu_download_weld_shells(p._ctx, None, 0, None, None) == soa.RET_SUCCESS  # no shells wanted
        p.weld()                                                                        # a re-weld invalidates
        assert no_shells(L, p._ctx)
        assert shells() == soa.RET_SUCCESS and not no_shells(L, p._ctx)
        p.set_model(model)                                                              # supersedes the run
        assert shells() == soa.RET_PARAM_ERROR and no_shells(L, p._ctx)
        p.polygonize(cs)
        assert shells() == soa.RET_PARAM_ERROR                                          # not finished
        p.finish()
        assert shells() == soa.RET_PARAM_ERROR and no_shells(L, p._ctx)                 # the weld was of the old run
        p.weld()
        assert p.weld_shells().info["ctShells"] == 2
    finally:
        p.close()


def test_group_shells_call_rules():
    """The group's rules, its runSeq ones included: whatever supersedes the group's run or its
    weld takes the shells with it."""
    L = gpu.load()
    info = gpu.PsShellsInfo()
    g = gpu.Group([0] * 3)
    try:
        shells = lambda: L.psgpu_group_weld_shells(g._g, ctypes.byref(info))  # noqa: E731
        none = lambda: no_shells(L, g._g, "psgpu_group_")  # noqa: E731
        assert shells() == soa.RET_PARAM_ERROR and none()                               # no run
        model, cs, _ = make_case("rand4_0.123457")
        g.set_model(model)
        g.run(cs)
        assert shells() == soa.RET_PARAM_ERROR and none()                               # a run, no weld
        g.weld()
        assert none()
        assert shells() == soa.RET_SUCCESS and info.ctShells == 2 and not none()
        buf = np.zeros(2, meshio.SHELL_DTYPE)
        assert L.psgpu_group_download_weld_shells(g._g, buf.ctypes.data, 1, None, None) == soa.RET_PARAM_ERROR
        g.weld()                                                                        # a re-weld invalidates
        assert none() and shells() == soa.RET_SUCCESS and not none()
        g.weld(1)                                                                       # ... so does one elsewhere
        assert none() and shells() == soa.RET_SUCCESS and not none()
        g.set_model(model)                                                              # supersedes the run
        assert shells() == soa.RET_PARAM_ERROR and none()
        g.run(cs)
        assert shells() == soa.RET_PARAM_ERROR and none()                               # the weld was of the old run
        g.weld()
        assert shells() == soa.RET_SUCCESS
        n = g.finish()[0].ctMPUs
        g.set_split([0, n // 3, 2 * n // 3, n])
        assert shells() == soa.RET_PARAM_ERROR and none()
        g.run(cs)
        g.weld()
        assert g.weld_shells().info["ctShells"] == 2
        g.set_option(gpu.OPT_CAPACITY, 1 << 20)                                         # the parts drop their runs
        assert shells() == soa.RET_PARAM_ERROR and none()
    finally:
        g.close()


def test_cpp_simdpoly_weld_shells(poly, tmp_path):
    """psgpu::SimdPolyGpu::weldShells() compiled as a host would compile it
    (tests/cpp/shells_check.cpp) on C1: PARAM_ERROR before the weld, then the same bytes as
    Polygonizer.weld_shells()."""
    gpp = shutil.which("g++")
    assert gpp is not None, "g++ is needed to compile the C++ face"
    lib_dir = os.path.join(ROOT, "parsip_amd")
    exe = tmp_path / "shells_check"
    subprocess.run([gpp, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shells_check.cpp"), "-L", lib_dir, "-l:libparsip_gpu.so",
                    f"-Wl,-rpath,{lib_dir}", "-o", str(exe)], check=True)
    model, cs, _ = make_case("C1")
    src, out = tmp_path / "soa.bin", tmp_path / "shells.bin"
    with open(src, "wb") as f:
        f.write(model.prims.tobytes() + model.mats.tobytes() + model.ops.tobytes())
    r = subprocess.run([str(exe), str(src), repr(float(cs)), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    rc = np.frombuffer(raw[:28], np.int32)
    assert rc[0] == soa.RET_PARAM_ERROR and (rc[1:] == soa.RET_SUCCESS).all(), rc
    assert raw[28:] == device_case(poly, "C1")[1].tobytes()
