"""The device weld filtered by shell (psgpu_weld_filter / psgpu_group_weld_filter,
parsip_amd/csrc/psgpu_filter.hip; DESIGN.md §6 "Filter"): byte for byte meshio.filter_shells of
the weld's and the shells' own downloads, the same bytes twice, a group against a context, and
the C-ABI's rules around the calls.  Thresholds come from tests/golden/shell_counts.json."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from parity_util import mesh_digests
from parsip_amd import gpu, meshio, soa, synth
from shells_util import golden_counts, make_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPPED = 0xFFFFFFFF
_RUNS = {}


def midway(name, field, a, b, absolute=False):
    per = golden_counts()[name]["per_shell"]
    x, y = per[a][field], per[b][field]
    if absolute:
        x, y = abs(x), abs(y)
    assert x != y
    return (x + y) / 2


# (input, criteria, mask, kept shells): C2 ~100 blocks, its 6-vertex shell dropped in the middle
# of the id space; the cavity; rand4's cut at vertex 403, inside a 256-lane block; rand1's two
# interleaved shells (waves with kept and dropped lanes), then both dropped; the non-manifold
# shell; the identity
def filter_cases():
    closed = {"flags": gpu.FILTER_CLOSED_ONLY}
    return {
        "C2": ("C2", {"minAbsVolume": midway("C2", "volume", 0, 2, absolute=True)}, None, [1, 1, 0]),
        "cavity": ("cube_minus_point", {"flags": gpu.FILTER_DROP_CAVITIES}, None, [1, 0]),
        "rand4": ("rand4_0.123457", {"minTriangles": int(midway("rand4_0.123457", "ctTriangles", 0, 1))}, None, [0, 1]),
        "rand1_mask": ("rand1_0.13", None, [0, 1], [0, 1]),
        "rand1_closed": ("rand1_0.13", closed, None, [0, 0]),
        "non_manifold": ("ring_union_point", closed, None, [0]),
        "identity": ("rand3_0.071_mpus_243_486", None, None, [1]),
    }


@pytest.fixture(scope="module")
def poly():
    assert gpu.device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"
    p = gpu.Polygonizer(0)
    yield p
    p.close()


def weld_bytes(w):
    return tuple(np.ascontiguousarray(a).tobytes() for a in (w.pos, w.nrm, w.col, w.tris, w.vertex_map))


def run_shells(p, name):
    model, cs, (b, e) = make_case(name)
    p.set_model(model)
    p.run(cs, b, e)
    w = p.weld()
    return w, p.weld_shells()


def device_case(poly, key):
    """(device weld, device shells, device filter, meshio.filter_shells of those downloads), once."""
    if key not in _RUNS:
        name, criteria, mask, _ = filter_cases()[key]
        w, sh = run_shells(poly, name)
        f = poly.weld_filter(criteria, mask)
        _RUNS[key] = (w, sh, f, meshio.filter_shells(w.pos, w.nrm, w.col, w.tris, sh, criteria, mask))
    return _RUNS[key]


def assert_same(got, want):
    """Array by array first (a readable failure), then every byte."""
    for a in ("pos", "nrm", "col", "tris", "vertex_map", "shell_map"):
        x, y = getattr(got, a), getattr(want, a)
        assert x.shape == y.shape and x.dtype == y.dtype, a
        assert x.tobytes() == y.tobytes(), a
    for f in meshio.SHELL_DTYPE.names:
        assert got.shells[f].tobytes() == want.shells[f].tobytes(), (f, got.shells[f], want.shells[f])
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("key", list(filter_cases()))
def test_filter_equals_host_form(poly, key):
    w, sh, f, ref = device_case(poly, key)
    kept = np.array(filter_cases()[key][3], bool)
    assert (f.shell_map != DROPPED).tolist() == kept.tolist()
    assert len(f.vertex_map) == len(w.pos) and len(f.shells) == int(kept.sum())
    assert len(f.pos) == int(sh.shells["ctVertices"][kept].sum())
    assert len(f.tris) == int(sh.shells["ctTriangles"][kept].sum())
    assert_same(f, ref)


def test_c2_loses_exactly_its_sliver(poly):
    w, sh, f, _ = device_case(poly, "C2")
    assert (len(w.pos) - len(f.pos), len(w.tris) - len(f.tris), len(f.shells)) == (6, 8, 2)
    assert len(w.pos) > 64 * 256        # ~100 blocks


def test_all_zero_filter_gives_the_welds_own_bytes(poly):
    w, sh, f, _ = device_case(poly, "identity")
    assert (f.pos.tobytes(), f.nrm.tobytes(), f.col.tobytes(), f.tris.tobytes()) == weld_bytes(w)[:4]
    assert np.array_equal(f.vertex_map, np.arange(len(w.pos))) and f.shells.tobytes() == sh.shells.tobytes()


def test_closed_only_of_open_shells_is_the_empty_mesh(poly):
    w, _, f, _ = device_case(poly, "rand1_closed")
    assert f.pos.shape == (0, 3) and f.tris.shape == (0, 3) and len(f.shells) == 0
    assert (f.vertex_map == DROPPED).all() and len(f.vertex_map) == len(w.pos)


def test_filter_twice_gives_the_same_bytes_and_disturbs_nothing(poly):
    """Two calls on one shells result: equal bytes; the weld's download, the shells' bytes and
    the run's mesh digests are what they were before the calls; the device pointers are set."""
    name, _, mask, _ = filter_cases()["rand1_mask"]
    model, cs, _ = make_case(name)
    poly.set_model(model)
    poly.run(cs)

    def digests():
        gm, gs = poly.download(), poly.stats()
        st = np.stack([gs["passedPrecheck"], gs["ctFieldEvals"], gs["ctVertices"], gs["ctTriangles"]], axis=1)
        return mesh_digests(st, gm.pos, gm.nrm, gm.col, gm.local_tris())

    def shells_bytes():
        n = len(sh.shells)
        buf, vs, ts = np.zeros(n, meshio.SHELL_DTYPE), np.zeros_like(sh.vertex_shell), np.zeros_like(sh.tri_shell)
        assert L.psgpu_download_weld_shells(poly._ctx, buf.ctypes.data, n, vs.ctypes.data,
                                            ts.ctypes.data) == soa.RET_SUCCESS
        return buf.tobytes() + vs.tobytes() + ts.tobytes()

    L = gpu.load()
    first = digests()
    w = poly.weld()
    sh = poly.weld_shells()
    before = shells_bytes()
    a = poly.weld_filter(mask=mask)
    d = poly.weld_filter_device()
    b = poly.weld_filter(mask=mask)
    assert a.tobytes() == b.tobytes() == device_case(poly, "rand1_mask")[2].tobytes()
    assert all(getattr(d, n) for n in ("pos", "nrm", "col", "tris", "vertexMap", "shellMap", "shells"))
    other = poly.weld_filter(mask=[1, 0])                   # a second call replaces the first
    assert other.tobytes() != a.tobytes() and other.shell_map.tolist() == [0, DROPPED]
    pos, tris = np.zeros_like(w.pos), np.zeros_like(w.tris)
    nrm, col, vmap = np.zeros_like(w.nrm), np.zeros_like(w.col), np.zeros_like(w.vertex_map)
    assert L.psgpu_download_weld(poly._ctx, pos.ctypes.data, nrm.ctypes.data, col.ctypes.data, tris.ctypes.data,
                                 vmap.ctypes.data) == soa.RET_SUCCESS
    assert weld_bytes(gpu.WeldedMesh(pos, nrm, col, tris, vmap, w.info)) == weld_bytes(w)
    assert shells_bytes() == before == sh.shells.tobytes() + sh.vertex_shell.tobytes() + sh.tri_shell.tobytes()
    assert digests() == first
    times = poly.weld_filter_times()
    assert len(times) == 7 and list(times)[0] == "filter total"


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("name", ["rand3_0.071", "rand1_0.13"])
def test_group_filter_equals_the_contexts(poly, name, k):
    """rand1 by mask, rand3 (one shell) by the all-zero filter and by one that drops it."""
    mask = [0, 1] if name == "rand1_0.13" else None
    w, sh = run_shells(poly, name)
    want = poly.weld_filter(mask=mask)
    none = poly.weld_filter({"minVertices": len(w.pos) + 1})
    assert_same(want, meshio.filter_shells(w.pos, w.nrm, w.col, w.tris, sh, None, mask))
    model, cs, _ = make_case(name)
    g = gpu.Group([0] * k)
    try:
        g.set_model(model)
        g.run(cs)
        g.weld()
        assert g.weld_shells().tobytes() == sh.tobytes()
        f = g.weld_filter(mask=mask)
        assert_same(f, want)
        d = g.weld_filter_device()
        assert d.pos and d.tris and d.vertexMap and d.shellMap and d.shells
        assert g.weld_filter(mask=mask).tobytes() == f.tobytes()
        assert_same(g.weld_filter({"minVertices": len(w.pos) + 1}), none)
        assert list(g.weld_filter_times())[0] == "filter total"
    finally:
        g.close()


def test_filter_of_an_empty_weld(poly):
    """A model whose surface lies outside the box: success and an empty mesh, on a context and a group."""
    model, cs, _ = synth.make_config("C1")
    model.prims["bboxLo"][0] = (5.0, 5.0, 5.0)
    model.prims["bboxHi"][0] = (6.0, 6.0, 6.0)
    poly.set_model(model)
    poly.run(cs)
    assert poly.weld().info.ctVertices == 0 and len(poly.weld_shells().shells) == 0
    for criteria in (None, {"flags": gpu.FILTER_CLOSED_ONLY, "minTriangles": 3}):
        f = poly.weld_filter(criteria)
        assert f.tobytes() == b"" and f.pos.shape == (0, 3)
    assert poly.weld_filter(mask=[]).tobytes() == b""
    info = gpu.PsFilterInfo()
    L = gpu.load()
    one = (ctypes.c_uint8 * 1)(1)
    assert L.psgpu_weld_filter(poly._ctx, None, one, 1, ctypes.byref(info)) == soa.RET_PARAM_ERROR   # 1 != 0 shells
    assert L.psgpu_weld_filter(poly._ctx, None, None, 0, ctypes.byref(info)) == soa.RET_SUCCESS
    assert bytes(info) == bytes(24)
    poly.weld_filter_device()
    g = gpu.Group([0] * 2)
    try:
        g.set_model(model)
        g.run(cs)
        g.weld()
        g.weld_shells()
        assert g.weld_filter().tobytes() == b""
    finally:
        g.close()


def no_filter(L, h, prefix="psgpu_"):
    d = gpu.PsFilterDevice()
    return (getattr(L, prefix + "weld_filter_device")(h, ctypes.byref(d)),
            getattr(L, prefix + "download_weld_filter")(h, None, None, None, None, None, None, None, 0)
            ) == (soa.RET_PARAM_ERROR,) * 2


def argument_rules(call, info):
    """What psgpu_weld_filter refuses of its arguments, on a 2-shell result; `call(f, mask, n, info)`."""
    F = gpu.PsShellFilter
    out, info = info, ctypes.byref(info)
    two, three = (ctypes.c_uint8 * 2)(0, 1), (ctypes.c_uint8 * 3)(1, 1, 1)
    assert call(None, two, 1, info) == soa.RET_PARAM_ERROR                              # a wrong maskCount
    assert call(None, three, 3, info) == soa.RET_PARAM_ERROR
    assert call(None, two, 0, info) == soa.RET_PARAM_ERROR
    assert call(ctypes.byref(F(flags=4)), None, 0, info) == soa.RET_PARAM_ERROR         # a bad flag
    assert call(ctypes.byref(F(flags=0x80000001)), None, 0, info) == soa.RET_PARAM_ERROR
    assert call(ctypes.byref(F(reserved=1)), None, 0, info) == soa.RET_PARAM_ERROR
    for bad in (float("nan"), float("inf"), -1.0):                                      # a NaN threshold
        assert call(ctypes.byref(F(minArea=bad)), None, 0, info) == soa.RET_PARAM_ERROR
        assert call(ctypes.byref(F(minAbsVolume=bad)), None, 0, info) == soa.RET_PARAM_ERROR
    assert call(ctypes.byref(F(flags=3, minArea=0.0)), two, 2, info) == soa.RET_SUCCESS
    assert (out.ctShells, out.ctInputShells) == (1, 2)


def test_filter_call_rules():
    L = gpu.load()
    p = gpu.Polygonizer(0)
    try:
        info = gpu.PsFilterInfo()
        call = lambda f, m, n, i: L.psgpu_weld_filter(p._ctx, f, m, n, i)  # noqa: E731
        flt = lambda: call(None, None, 0, ctypes.byref(info))  # noqa: E731
        assert flt() == soa.RET_PARAM_ERROR and no_filter(L, p._ctx)                    # no run yet
        model, cs, _ = make_case("rand4_0.123457")
        p.set_model(model)
        p.run(cs)
        assert flt() == soa.RET_PARAM_ERROR and no_filter(L, p._ctx)                    # a run, no weld
        p.weld()
        assert flt() == soa.RET_PARAM_ERROR and no_filter(L, p._ctx)                    # a weld, no shells
        p.weld_shells()
        assert no_filter(L, p._ctx)                                                     # shells, no filter call
        with pytest.raises(gpu.PsgpuError):
            p.weld_filter_device()
        assert flt() == soa.RET_SUCCESS and info.ctShells == 2 and not no_filter(L, p._ctx)
        assert (info.ctVertices, info.ctTriangles) == (info.ctInputVertices, info.ctInputTriangles) == (1654, 3300)
        assert call(None, None, 0, None) == soa.RET_SUCCESS                             # info may be NULL
        argument_rules(call, info)
        assert not no_filter(L, p._ctx)
        assert call(ctypes.byref(gpu.PsShellFilter(flags=4)), None, 0, None) == soa.RET_PARAM_ERROR
        assert not no_filter(L, p._ctx)                                                 # ... and the result stays
        assert flt() == soa.RET_SUCCESS and info.ctShells == 2
        buf = np.zeros(2, meshio.SHELL_DTYPE)
        dl = lambda cap: L.psgpu_download_weld_filter(p._ctx, None, None, None, None, None, None,  # noqa: E731
                                                      buf.ctypes.data, cap)
        assert dl(1) == soa.RET_PARAM_ERROR and dl(2) == soa.RET_SUCCESS                # a short shellCapacity
        assert buf["firstVertex"].tolist() == [0, 403]
        p.weld_shells()                                                                 # a new shells call invalidates
        assert no_filter(L, p._ctx) and flt() == soa.RET_SUCCESS and not no_filter(L, p._ctx)
        p.weld()                                                                        # a re-weld invalidates
        assert flt() == soa.RET_PARAM_ERROR and no_filter(L, p._ctx)
        p.weld_shells()
        assert flt() == soa.RET_SUCCESS and not no_filter(L, p._ctx)
        p.set_model(model)                                                              # supersedes the run
        assert flt() == soa.RET_PARAM_ERROR and no_filter(L, p._ctx)
        p.run(cs)
        assert flt() == soa.RET_PARAM_ERROR and no_filter(L, p._ctx)                    # the weld was of the old run
        p.weld()
        p.weld_shells()
        assert len(p.weld_filter().shells) == 2
    finally:
        p.close()


def test_group_filter_call_rules():
    L = gpu.load()
    info = gpu.PsFilterInfo()
    g = gpu.Group([0] * 3)
    try:
        call = lambda f, m, n, i: L.psgpu_group_weld_filter(g._g, f, m, n, i)  # noqa: E731
        flt = lambda: call(None, None, 0, ctypes.byref(info))  # noqa: E731
        none = lambda: no_filter(L, g._g, "psgpu_group_")  # noqa: E731
        assert flt() == soa.RET_PARAM_ERROR and none()                                  # no run
        model, cs, _ = make_case("rand4_0.123457")
        g.set_model(model)
        g.run(cs)
        assert flt() == soa.RET_PARAM_ERROR and none()                                  # a run, no weld
        g.weld()
        assert flt() == soa.RET_PARAM_ERROR and none()                                  # a weld, no shells
        g.weld_shells()
        assert none() and flt() == soa.RET_SUCCESS and info.ctShells == 2 and not none()
        assert call(None, None, 0, None) == soa.RET_SUCCESS                             # info may be NULL
        argument_rules(call, info)
        buf = np.zeros(2, meshio.SHELL_DTYPE)
        assert L.psgpu_group_download_weld_filter(g._g, None, None, None, None, None, None, buf.ctypes.data,
                                                  0) == soa.RET_PARAM_ERROR             # a short shellCapacity
        g.weld_shells()                                                                 # a new shells call invalidates
        assert none() and flt() == soa.RET_SUCCESS and not none()
        g.weld(1)                                                                       # a re-weld, elsewhere
        assert flt() == soa.RET_PARAM_ERROR and none()
        g.weld_shells()
        assert flt() == soa.RET_SUCCESS and not none()
        g.set_model(model)                                                              # supersedes the run
        assert flt() == soa.RET_PARAM_ERROR and none()
        g.run(cs)
        g.weld()
        g.weld_shells()
        assert len(g.weld_filter().shells) == 2
    finally:
        g.close()


def test_filter_buffers_go_with_the_context_and_the_group():
    base = gpu.device_bytes()
    model, cs, _ = make_case("rand4_0.123457")
    p = gpu.Polygonizer(0)
    try:
        p.set_model(model)
        p.run(cs)
        p.weld()
        p.weld_shells()
        before = gpu.device_bytes()
        assert len(p.weld_filter(mask=[1, 0]).shells) == 1
        assert gpu.device_bytes() > before > base
    finally:
        p.close()
    assert gpu.device_bytes() == base
    g = gpu.Group([0] * 2)
    try:
        g.set_model(model)
        g.run(cs)
        g.weld()
        g.weld_shells()
        before = gpu.device_bytes()
        assert len(g.weld_filter(mask=[1, 0]).shells) == 1
        assert gpu.device_bytes() > before
    finally:
        g.close()
    assert gpu.device_bytes() == base


def test_cpp_simdpoly_weld_filter(poly, tmp_path):
    """psgpu::SimdPolyGpu::weldFilter() compiled as a host would compile it
    (tests/cpp/filter_check.cpp) on C1 with the all-zero filter: PARAM_ERROR before the shells,
    then the same bytes as Polygonizer.weld_filter()."""
    gpp = shutil.which("g++")
    assert gpp is not None, "g++ is needed to compile the C++ face"
    lib_dir = os.path.join(ROOT, "parsip_amd")
    exe = tmp_path / "filter_check"
    subprocess.run([gpp, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "filter_check.cpp"), "-L", lib_dir, "-l:libparsip_gpu.so",
                    f"-Wl,-rpath,{lib_dir}", "-o", str(exe)], check=True)
    model, cs, _ = make_case("C1")
    src, out = tmp_path / "soa.bin", tmp_path / "filter.bin"
    with open(src, "wb") as f:
        f.write(model.prims.tobytes() + model.mats.tobytes() + model.ops.tobytes())
    r = subprocess.run([str(exe), str(src), repr(float(cs)), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    rc = np.frombuffer(raw[:32], np.int32)
    assert rc[0] == soa.RET_PARAM_ERROR and (rc[1:] == soa.RET_SUCCESS).all(), rc
    w, _ = run_shells(poly, "C1")
    want = poly.weld_filter()
    assert len(want.pos) == len(w.pos) > 0
    assert raw[32:] == want.tobytes()
