"""The compat mode's weld, shells and filter on the device (psgpu_gui_weld and its family,
parsip_amd/csrc/psgpu_gui.hip; DESIGN.md §6 "Compat weld"): k_gui_weld_edges against
gui.lattice_edges, the weld byte for byte against meshio.weld_by_edges, the shells against
meshio.shells, the filter against meshio.filter_shells with rgba colours (the 4-wide
k_weld_emit / k_filter_emit), the same bytes twice and under both kernel sets, the C-ABI's rules
around the calls, and one hot-path case through the 3-wide instantiations.  The inputs are the six
small lattices of tests/gui_weld_util.py; a case runs once and its results are shared."""
import numpy as np
import pytest

from gui_weld_util import CASES, ISO, degenerate_count, golden, lattice_dims, make_tree
from parsip_amd import blobtree as bt
from parsip_amd import gpu, gui, meshio, soa, synth

pytestmark = pytest.mark.gpu

B = bt.BlobNodeType
DROPPED = 0xFFFFFFFF
CLOSED = {"flags": gpu.FILTER_CLOSED_ONLY}
_RUNS = {}


@pytest.fixture(scope="module")
def ctx():
    assert gpu.device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"
    p = gui.ParsipOptimized(0, jit=0)
    yield p
    p.close()


def run_case(p, name):
    """setup + run of a named input from the state a fresh tree starts with; returns the mesh."""
    tree, cs = make_tree(name)
    p.setup(tree, cellsize=cs, isovalue=ISO)
    p.set_pcm_state((ISO, ISO))  # what set_tree leaves; the tree objects are shared between runs
    p.run()
    return p.exportMesh()


def host_edges(p, name, mesh):
    """gui.lattice_edges of a download with the device's own field, probed with the contact state
    the run started from."""
    tree, cs = make_tree(name)
    after = p.pcm_state
    p.set_pcm_state((ISO, ISO))
    e = gui.lattice_edges(mesh, lattice_dims(tree, cs), tree.root_octree[0], cs, ISO, lambda x: p.field_values(x)[0])
    p.set_pcm_state(after)
    return e


def tri_mesh(mesh):
    return meshio.TriMesh(mesh.pos, mesh.tris.astype(np.int64), mesh.nrm, mesh.col)


def weld_bytes(w):
    return tuple(np.ascontiguousarray(a).tobytes() for a in (w.pos, w.nrm, w.col, w.tris, w.vertex_map))


def device_case(p, name):
    """One run of a named input on the module's context: the download, the device's edges and
    the host's, the device weld and shells, and the filters (all-zero, closed only, and a mask
    without shell 0 where there are two shells) with their host forms, computed once."""
    if name not in _RUNS:
        mesh = run_case(p, name)
        edges = p.vertex_edges()
        w = p.weld()
        sh = p.weld_shells()
        filters = {"zero": (None, None), "closed": (CLOSED, None)}
        if len(sh.shells) == 2:
            filters["mask"] = (None, [0, 1])
        got = {k: p.weld_filter(c, m) for k, (c, m) in filters.items()}
        want = {k: meshio.filter_shells(w.pos, w.nrm, w.col, w.tris, sh, c, m) for k, (c, m) in filters.items()}
        _RUNS[name] = dict(mesh=mesh, edges=edges, host_edges=host_edges(p, name, mesh), weld=w, shells=sh,
                           filters=got, host_filters=want)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_vertex_edges_equal_host_form(ctx, name):
    """psgpu_gui_download_edges (k_gui_weld_edges, every vertex, interior ones included) equals
    gui.lattice_edges of the same download with field = the context's field_values."""
    r = device_case(ctx, name)
    gold = golden()["cases"][name]
    assert (len(r["mesh"].pos), len(r["mesh"].tris)) == (gold["vertices"], gold["triangles"])
    assert r["edges"].dtype == np.uint32 and r["edges"].shape == (gold["vertices"], 4)
    assert np.array_equal(r["edges"].astype(np.int64), r["host_edges"])


@pytest.mark.parametrize("name", list(CASES))
def test_weld_equals_host_form(ctx, name):
    """weld() is byte-equal to meshio.weld_by_edges(exportMesh(), edges): positions, normals,
    rgba, triangles and vertexMap; its counts are the golden file's."""
    r = device_case(ctx, name)
    mesh, w, gold = r["mesh"], r["weld"], golden()["cases"][name]
    ref, ref_map = meshio.weld_by_edges(tri_mesh(mesh), r["host_edges"])
    e = r["host_edges"]
    off = np.ones((len(e), 3), bool)
    off[np.arange(len(e)), e[:, 3]] = False
    seam = ((e[:, :3] % 7 == 0) & off).any(axis=1)
    assert (w.info.ctVertices, w.info.ctTriangles, w.info.ctInputVertices, w.info.ctSeamVertices) == \
        (ref.n_vertices, len(mesh.tris), len(mesh.pos), int(seam.sum()))
    assert w.info.ctVertices == gold["edge_weld"]["vertices"]
    assert w.col.shape == (ref.n_vertices, 4)
    for what, got, want in (("pos", w.pos, ref.pos), ("nrm", w.nrm, ref.nrm), ("col", w.col, ref.col)):
        assert got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want, np.float32).tobytes(), what
    assert np.array_equal(w.tris, ref.tris.astype(np.uint32))
    assert np.array_equal(w.vertex_map, ref_map.astype(np.uint32))
    assert degenerate_count(w.tris) == 0
    assert meshio.open_edge_count(w.tris) == gold["edge_weld"]["open_edges"]


@pytest.mark.parametrize("name", list(CASES))
def test_shells_equal_host_form(ctx, name):
    r = device_case(ctx, name)
    w, sh, gold = r["weld"], r["shells"], golden()["cases"][name]["edge_weld"]
    ref = meshio.shells(w.pos, w.tris)
    for f in meshio.SHELL_DTYPE.names:
        assert sh.shells[f].tobytes() == ref.shells[f].tobytes(), (f, sh.shells[f], ref.shells[f])
    assert sh.tobytes() == ref.tobytes()
    assert (len(sh.shells), [int(x) for x in sh.shells["euler"]]) == (gold["shells"], gold["euler"])


def assert_filter_same(got, want):
    for a in ("pos", "nrm", "col", "tris", "vertex_map", "shell_map"):
        x, y = getattr(got, a), getattr(want, a)
        assert x.shape == y.shape and x.dtype == y.dtype, (a, x.shape, y.shape, x.dtype, y.dtype)
        assert x.tobytes() == y.tobytes(), a
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_filters_equal_host_form(ctx, name):
    """The all-zero filter (the weld's own bytes) and `closed only` on every input."""
    r = device_case(ctx, name)
    w, sh = r["weld"], r["shells"]
    for k in ("zero", "closed"):
        assert_filter_same(r["filters"][k], r["host_filters"][k])
    z = r["filters"]["zero"]
    assert z.col.shape == (len(w.pos), 4)
    assert (z.pos.tobytes(), z.nrm.tobytes(), z.col.tobytes(), z.tris.tobytes()) == weld_bytes(w)[:4]
    assert np.array_equal(z.vertex_map, np.arange(len(w.pos))) and z.shells.tobytes() == sh.shells.tobytes()


@pytest.mark.parametrize("name", ["random3_cs0.13", "random5_cs0.1"])
def test_mask_drops_shell_0(ctx, name):
    """Two shells, the mask keeps the second: kept and dropped lanes in the same blocks."""
    r = device_case(ctx, name)
    f, sh = r["filters"]["mask"], r["shells"]
    assert_filter_same(f, r["host_filters"]["mask"])
    assert f.shell_map.tolist() == [DROPPED, 0]
    assert 0 < len(f.pos) == int(sh.shells["ctVertices"][1]) < len(r["weld"].pos)
    assert len(f.tris) == int(sh.shells["ctTriangles"][1])


def test_closed_only_of_random3(ctx):
    """random_tree(3, ...) has open seams towards MPUs the octree test skipped: `closed only`
    keeps exactly its closed shells, here none."""
    r = device_case(ctx, "random3_cs0.13")
    f, sh = r["filters"]["closed"], r["shells"].shells
    closed = (sh["ctOpenEdges"] == 0) & (sh["ctFlippedEdges"] == 0) & (sh["ctNonManifoldEdges"] == 0)
    assert (f.shell_map != DROPPED).tolist() == closed.tolist()
    assert not closed.all() and len(f.pos) == int(sh["ctVertices"][closed].sum())


def test_two_welds_of_one_run_give_the_same_bytes(ctx):
    run_case(ctx, "random5_cs0.1")
    w1, s1 = ctx.weld(), ctx.weld_shells()
    f1 = ctx.weld_filter(None, [0, 1])
    d1 = ctx.weld_device()
    w2, s2 = ctx.weld(), ctx.weld_shells()
    f2 = ctx.weld_filter(None, [0, 1])
    assert weld_bytes(w1) == weld_bytes(w2) and s1.tobytes() == s2.tobytes() and f1.tobytes() == f2.tobytes()
    assert weld_bytes(w1) == weld_bytes(device_case(ctx, "random5_cs0.1")["weld"])
    assert all(getattr(d1, n) for n in ("pos", "nrm", "col", "tris", "vertexMap"))
    fd, sd = ctx.weld_filter_device(), ctx.weld_shells_device()
    assert all(getattr(fd, n) for n in ("pos", "nrm", "col", "tris", "vertexMap", "shellMap", "shells"))
    assert all(getattr(sd, n) for n in ("shells", "vertexShell", "triShell"))


def test_interpreter_and_generated_kernels_give_the_same_bytes(ctx):
    """jit=0 (the module's context) and jit=2 (the tree's generated kernels, waited for)."""
    name = "random3_cs0.13"
    r = device_case(ctx, name)
    p = gui.ParsipOptimized(0, jit=2)
    try:
        run_case(p, name)
        assert p.jit_status() == gui.JIT_ACTIVE
        assert np.array_equal(p.vertex_edges(), r["edges"])
        assert weld_bytes(p.weld()) == weld_bytes(r["weld"])
        assert p.weld_shells().tobytes() == r["shells"].tobytes()
        assert p.weld_filter(None, [0, 1]).tobytes() == r["filters"]["mask"].tobytes()
    finally:
        p.close()


def test_timing_option_reports_the_phases(ctx):
    run_case(ctx, "sphere_cs0.071")
    ctx.set_timing(True)
    try:
        ctx.weld_info()
        ctx.weld_shells()
        ctx.weld_filter()
        t = ctx.weld_times()
        assert list(t)[0] == "weld total" and list(t)[-1] == "k_gui_weld_edges" and len(t) == 7
        assert t["weld total"] > 0.0 and t["k_weld_emit"] > 0.0 and t["k_gui_weld_edges"] > 0.0
        assert ctx.weld_shells_times()["shells total"] > 0.0 and ctx.weld_filter_times()["filter total"] > 0.0
    finally:
        ctx.set_timing(False)
    ctx.weld_info()
    assert all(v == 0.0 for v in ctx.weld_times().values())


def _param_error(fn, *a):
    with pytest.raises(gpu.PsgpuError) as e:
        fn(*a)
    assert e.value.code == soa.RET_PARAM_ERROR


def test_error_paths():
    """No weld before finish, none of a superseded run; no shells before the weld, no filter before
    the shells; device pointers and downloads follow."""
    tree, cs = make_tree("sphere_cs0.13")
    p = gui.ParsipOptimized(0, jit=0)
    try:
        _param_error(p.weld_info)                       # no run at all
        p.setup(tree, cellsize=cs, isovalue=ISO)
        _param_error(p.weld_info)                       # a tree, no run
        p.polygonize()
        _param_error(p.weld_info)                       # enqueued, not finished
        e = np.zeros((1024, 4), np.uint32)
        assert p._L.psgpu_gui_download_edges(p._g, e.ctypes.data) == soa.RET_PARAM_ERROR
        p.finish()
        _param_error(p.weld_shells)                     # shells before weld
        _param_error(p.weld_device)
        assert p.weld_info().ctVertices == 234
        _param_error(p.weld_filter)                     # filter before shells
        _param_error(p.weld_shells_device)
        assert p.weld_shells().info["ctShells"] == 1
        _param_error(p.weld_filter_device)
        assert len(p.weld_filter().pos) == 234
        bad = meshio.shell_filter()
        bad["flags"] = 4                                # an unknown flag: refused, the result stays
        assert p._L.psgpu_gui_weld_filter(p._g, bad.ctypes.data, None, 0, None) == soa.RET_PARAM_ERROR
        assert p.weld_filter_device().pos
        p.weld_info()                                   # a new weld drops its shells and filter
        _param_error(p.weld_filter)
        _param_error(p.weld_shells_device)
        p.polygonize()                                  # a newer run supersedes the weld
        _param_error(p.weld_info)
        _param_error(p.weld_device)
        p.finish()
        _param_error(p.weld_device)                     # finished, not welded yet
        _param_error(p.weld_shells)
        assert p.weld_info().ctVertices == 234
        p.set_tree(make_tree("sphere_cs0.3")[0])        # a new tree supersedes the run
        _param_error(p.weld_info)
        _param_error(p.weld_device)
        assert p._L.psgpu_gui_weld(None, None) == soa.RET_PARAM_ERROR
    finally:
        p.close()


def test_empty_mesh_welds_to_zero_counts(ctx):
    """An all-Null tree: over its own (empty) octree the lattice has no MPU; over a given box it
    has MPUs and no vertex.  Both weld to zero counts, no shell, an empty filter."""
    code, tree = gui.compact_blobtree(bt.Op(B.OP_UNION, bt.Null(), bt.Null()))
    assert code >= 0
    for octree in (None, ((-0.5, -0.5, -0.5), (0.5, 0.3, 0.5))):
        ctx.setup(tree, octree=octree, cellsize=0.1, isovalue=ISO)
        info = ctx.run()
        assert info.ctVertices == 0 and (info.ctLatticeMPUs > 0) == (octree is not None)
        assert ctx.vertex_edges().shape == (0, 4)
        w = ctx.weld()
        assert (w.info.ctVertices, w.info.ctTriangles, w.info.ctInputVertices, w.info.ctSeamVertices) == (0, 0, 0, 0)
        assert w.pos.shape == (0, 3) and w.col.shape == (0, 4) and len(w.vertex_map) == 0
        assert len(ctx.weld_shells().shells) == 0
        f = ctx.weld_filter()
        assert f.pos.shape == (0, 3) and f.col.shape == (0, 4) and len(f.shells) == 0


def test_close_releases_every_byte(ctx):
    """psgpu_debug_device_bytes() after close() is what it was before the context was made."""
    before = gpu.device_bytes()
    p = gui.ParsipOptimized(0, jit=0)
    run_case(p, "random5_cs0.1")
    p.set_timing(True)
    p.vertex_edges()
    p.weld()
    p.weld_shells()
    p.weld_filter(None, [0, 1])
    assert gpu.device_bytes() > before
    p.close()
    assert gpu.device_bytes() == before


def test_hot_path_weld_and_filter_unchanged():
    """C1 through Polygonizer.weld() / weld_shells() / weld_filter(): byte-equal to its host
    forms, as before: the 3-wide k_weld_emit / k_filter_emit beside the 4-wide ones."""
    model, cs, _ = synth.make_config("C1")
    poly = gpu.Polygonizer(0)
    try:
        poly.set_model(model)
        poly.run(cs)
        mesh = poly.download()
        w = poly.weld()
        ref, ref_map = meshio.weld_lattice(mesh, mesh.vertex_offsets, cs, *model.bbox)
        assert w.col.shape == (ref.n_vertices, 3) and ref.n_vertices == 1014
        for got, want in ((w.pos, ref.pos), (w.nrm, ref.nrm), (w.col, ref.col)):
            assert got.tobytes() == np.ascontiguousarray(want, np.float32).tobytes()
        assert np.array_equal(w.tris, ref.tris.astype(np.uint32))
        assert np.array_equal(w.vertex_map, ref_map.astype(np.uint32))
        sh = poly.weld_shells()
        assert sh.tobytes() == meshio.shells(w.pos, w.tris).tobytes()
        for crit, mask in ((None, None), (CLOSED, None), (None, [0] * len(sh.shells))):
            f = poly.weld_filter(crit, mask)
            assert_filter_same(f, meshio.filter_shells(w.pos, w.nrm, w.col, w.tris, sh, crit, mask))
            assert f.col.shape[1] == 3
    finally:
        poly.close()
