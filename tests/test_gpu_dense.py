"""Dense MPUs on the HIP path (tests/dense_util.py: over 512 and up to 1,344 vertices, 1,372
triangles per MPU) against the CPU oracle, bit for bit: local ids past 1,024 through k_mpu's
packed records (TriRec's tlocal bit 10, v0 / v1 bit 10 and the split v2 bit, VertexKey's vid,
the S3 carry V | T << 16, find_cell over full tables), block reservations of several x 1,344
records in one shard and the grow-and-rerun behind them, k_vertex / k_finish / k_surface
batches filled from one MPU -- and the overflow contract of include/parsip_gpu.h
(PsMeshInfo.firstOverflowMPU, PSGPU_RET_MPU_VT_OVERFLOW, psgpu_weld's PARAM_ERROR).
Every case is one run of at most 8 MPUs."""
import contextlib
import ctypes
import time

import numpy as np
import pytest

import dense_util as du
from parity_util import assert_bits_equal, assert_mesh_matches, mesh_digests
from parsip_amd import gpu, meshio, soa, synth

pytestmark = pytest.mark.gpu

CS = du.CS
DEFAULTS = {gpu.OPT_CULLING: 1, gpu.OPT_JIT: 1, gpu.OPT_VERTEX_WIDE: 2, gpu.OPT_FINISH_QUAD: 2,
            gpu.OPT_TREE_SPLIT: 0, gpu.OPT_FUSED_SURFACE: 2, gpu.OPT_FRONT: 2, gpu.OPT_OP_INSIDE: 1,
            gpu.OPT_GRAPH: 0}
S, F, R, X = gpu.LAUNCH_TREE_SPLIT, gpu.LAUNCH_SURFACE, gpu.LAUNCH_FRONT, gpu.LAUNCH_RERUN
# variant -> (options, launch flags the run must report, flags it must not, runs)
VARIANTS = {
    "default": ({}, 0, S, 2),
    "surface": ({gpu.OPT_FUSED_SURFACE: 1}, F, S, 2),  # the unsplit k_surface (always generated)
    "vertex16_finish64": ({gpu.OPT_VERTEX_WIDE: 0, gpu.OPT_FINISH_QUAD: 0, gpu.OPT_FUSED_SURFACE: 0}, 0, F, 2),
    "vertex64_finish16": ({gpu.OPT_VERTEX_WIDE: 1, gpu.OPT_FINISH_QUAD: 1, gpu.OPT_FUSED_SURFACE: 0}, 0, F, 2),
    "finish32": ({gpu.OPT_FINISH_QUAD: 3, gpu.OPT_FUSED_SURFACE: 0}, 0, F, 2),
    "front0": ({gpu.OPT_FRONT: 0}, 0, R, 2),
    "front1": ({gpu.OPT_FRONT: 1}, R, 0, 2),
    "culling0": ({gpu.OPT_CULLING: 0}, 0, 0, 2),
    "op_inside0": ({gpu.OPT_OP_INSIDE: 0}, 0, 0, 2),
    # each of the context's two counter sets (runs alternate between them) has a graph of its own,
    # keyed by the run's parameters: run 1 may still size its grids without a finished run or be
    # re-run by finish, runs 2-3 capture both sets' graphs on the warmed context, runs 4-6 relaunch them
    "graph": ({gpu.OPT_GRAPH: 1}, 0, 0, 6),
    "split": ({gpu.OPT_TREE_SPLIT: 1, gpu.OPT_FUSED_SURFACE: 0}, S, F, 2),
    "split_surface": ({gpu.OPT_TREE_SPLIT: 1, gpu.OPT_FUSED_SURFACE: 1}, S | F, 0, 2),
    "split_surface_wide": ({gpu.OPT_TREE_SPLIT: 1, gpu.OPT_FUSED_SURFACE: 3}, S | F, 0, 2),
    "split_front1": ({gpu.OPT_TREE_SPLIT: 1, gpu.OPT_FRONT: 1}, S | R, 0, 2),
}


@pytest.fixture(scope="module")
def poly():
    """A context of this module's own (the tests below change its options)."""
    assert gpu.device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"
    p = gpu.Polygonizer(0)
    yield p
    p.close()


@contextlib.contextmanager
def interpreter(p, on=True):
    """The context on the interpreter kernels (OPT_JIT 0).  It goes back to the generated kernels
    with C1 as its model: OPT_JIT 1 compiles the current model's kernels, and those of a
    128-primitive tree take minutes of hiprtc."""
    p.set_option(gpu.OPT_JIT, 0 if on else 1)
    try:
        yield p
    finally:
        if on:
            p.set_option(gpu.OPT_JIT, 0)
            p.set_model(synth.make_config("C1")[0], wait_jit=False)
        p.set_option(gpu.OPT_JIT, 1)


def set_options(p, opts):
    for k, v in opts.items():
        p.set_option(k, v)


def run_and_compare(p, oracle, name, begin=0, end=None, runs=2, need=0, never=0, tag=""):
    """Upload `name`, run its MPUs [begin, end) `runs` times on the context as it is set up (the
    first run may have to grow the buffers and re-run: LAUNCH_RERUN is expected there; the later
    ones run on the warmed context) and compare every run's final result with the oracle's."""
    om = du.oracle_mesh(oracle, name, begin, 0xFFFFFFFF if end is None else end)
    p.set_model(du.model_of(name))
    flagged = np.flatnonzero(om.stats[:, 4])
    infos = []
    for k in range(runs):
        info = p.run(CS, begin, end)
        infos.append(info)
        assert_mesh_matches(p.download(), p.stats(), om)
        assert (info.ctMPUs, info.ctVertices, info.ctTriangles) == (len(om.stats), len(om.pos), len(om.tris))
        assert info.firstOverflowMPU == (begin + int(flagged[0]) if len(flagged) else -1)
        assert info.launchFlags & need == need and not info.launchFlags & never, (name, tag, k, info.launchFlags)
    assert not infos[-1].launchFlags & X, "a warmed context re-ran"
    print(f"dense {name} {tag}: V {om.stats[:, 2].tolist()} T {om.stats[:, 3].tolist()} "
          f"launchFlags {[i.launchFlags for i in infos]}")
    return infos, om


# ---- 1. the compact mesh, every kernel family -------------------------------------------
@pytest.mark.parametrize("name", ["checker", "checker2x1x1", "checker1x1x2", *du.RAND_NAMES, "mixed", "below"])
def test_interpreter_matches_oracle(poly, oracle, name):
    """The interpreter kernels (88 to 128 primitives: no hiprtc compile the suite has not paid for)."""
    with interpreter(poly):
        run_and_compare(poly, oracle, name, tag="interp")
        assert not poly.jit_active


@pytest.mark.parametrize("fquad", [0, 1, 3])
def test_interpreter_off_segment_roots_every_finish_layout(poly, oracle, fquad):
    """Roots off their bracketing segments (randlines31: the bracket hits fb == fa, NaN positions)
    through k_finish itself, 64 / 16 / 32 vertices per wave: a wave that holds one takes the
    culling mask of its own points' box instead of its MPUs' masks."""
    name = "randlines%d" % du.NAN_SEED
    assert not np.isfinite(du.oracle_mesh(oracle, name).pos).all(), "no off-segment root in the oracle's mesh"
    opts = {gpu.OPT_FUSED_SURFACE: 0, gpu.OPT_FINISH_QUAD: fquad}
    try:
        set_options(poly, opts)
        with interpreter(poly):
            run_and_compare(poly, oracle, name, never=F, tag=f"interp finish_quad {fquad}")
            assert not poly.jit_active
    finally:
        set_options(poly, {k: DEFAULTS[k] for k in opts})


def test_checker_generated_kernels(poly, oracle):
    """V = 1,344 / T = 1,372 through the structure-specialised kernels of the 60-primitive tree."""
    t0 = time.perf_counter()
    poly.set_model(du.model_of("checker"))
    assert poly.jit_active
    print(f"dense checker: set_model + hiprtc {time.perf_counter() - t0:.1f} s")
    run_and_compare(poly, oracle, "checker", tag="jit")


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["zlines", "randlines32"])
def test_generated_kernel_matrix(poly, oracle, name, variant):
    """The options the fuzz test draws from, on 32-primitive dense trees (zlines: one MPU of
    896 / 1,372; randlines32: two MPUs with a seam) with the generated kernels."""
    opts, need, never, runs = VARIANTS[variant]
    try:
        set_options(poly, opts)
        poly.set_model(du.model_of(name))
        assert poly.jit_active
        run_and_compare(poly, oracle, name, runs=runs, need=need, never=never, tag=variant)
    finally:
        set_options(poly, {k: DEFAULTS[k] for k in opts})


# ---- 2. capacity ---------------------------------------------------------------------
def test_capacity_64_reruns_to_the_same_bytes(poly, oracle):
    """Two MPUs of 1,344 vertices in one k_mpu block (one reservation of 2,688 records in one
    shard: asserted on the vertex queue) against buffers started at 64 vertices: finish grows
    them and re-runs."""
    def one_reservation(p):
        counts, shards = p.vertex_queue()
        assert sorted(counts.tolist())[-2:] == [0, 2688], counts
        recs = shards[int(counts.argmax())]  # the block's MPUs back to back, each in vid order
        assert recs[:, 1].tolist() == 2 * list(range(1344)) and sorted(set(recs[:, 0].tolist())) == [0, 1]
        assert (np.diff(recs[:, 0]) != 0).sum() == 1

    with interpreter(poly):
        run_and_compare(poly, oracle, "checker2x1x1", tag="interp")
        want = poly.download()
        one_reservation(poly)
    p = gpu.Polygonizer(0)
    try:
        p.set_option(gpu.OPT_JIT, 0)
        p.set_option(gpu.OPT_CAPACITY, 64)
        infos, _ = run_and_compare(p, oracle, "checker2x1x1", tag="capacity64")
        assert infos[0].launchFlags & X
        got = p.download()
        one_reservation(p)
        for f in ("pos", "nrm", "col", "tris", "vertex_offsets", "triangle_offsets"):
            assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f
    finally:
        p.close()


# ---- 3. a sub-range -------------------------------------------------------------------
@pytest.mark.parametrize("name,begin,end", [(du.RAND_NAMES[1], 3, 8), ("mixed", 3, 8), ("mixed", 5, 7), ("mixed", 0, 4)])
def test_sub_range(poly, oracle, name, begin, end):
    """MPUs [begin, end): the oracle's mesh of that range, and firstOverflowMPU the smallest
    global id in the range that the oracle flags (mixed flags 4 and 7: [5, 7) and [0, 4) hold none)."""
    with interpreter(poly):
        infos, om = run_and_compare(poly, oracle, name, begin, end, tag=f"interp[{begin},{end})")
        full = du.oracle_mesh(oracle, name).stats[:, 4]
        hit = [m for m in range(begin, end) if full[m]]
        assert infos[-1].firstOverflowMPU == (hit[0] if hit else -1)


# ---- 4. the overflow contract ---------------------------------------------------------
def _c1_succeeds(call):
    """C1 through `call(cellsize, model, mpus)` -> (rc, ct): success, so no flag sticks."""
    model, cs, _ = synth.make_config("C1")
    n = gpu.count_mpus(cs, *model.bbox)
    mpus = np.zeros(n, soa.MPU_DTYPE)
    rc, ct = call(cs, model, mpus)
    assert rc == soa.RET_SUCCESS and ct == n
    assert (int(mpus["ctVertices"].sum()), int(mpus["ctTriangles"].sum())) == (1326, 2024)


@pytest.mark.parametrize("name", [n for n in du.INPUTS if n != "below"])
def test_overflow_is_reported_not_exported(poly, oracle, name):
    """run() succeeds and finish() reports the smallest flagged MPU in firstOverflowMPU; the
    blocking export returns PSGPU_RET_MPU_VT_OVERFLOW with outCt filled and leaves the caller's
    PolyMPUs (512 slots per MPU) untouched, the mpus-null count check returns the same code; C1
    on the same context afterwards succeeds with firstOverflowMPU -1."""
    L = gpu.load()
    om = du.oracle_mesh(oracle, name)
    first = int(np.flatnonzero(om.stats[:, 4])[0])
    model = du.model_of(name)
    n = len(om.stats)
    with interpreter(poly, on=model.ct_prims > 32):
        poly.set_model(model)
        info = poly.run(CS)
        assert info.firstOverflowMPU == first
        ct = ctypes.c_uint32(0xDEAD)
        mpus = np.zeros(n, soa.MPU_DTYPE)
        assert L.psgpu_export_polympus(poly._ctx, mpus.ctypes.data, n, ctypes.byref(ct)) == soa.RET_MPU_VT_OVERFLOW
        assert ct.value == n and not mpus.view(np.uint8).any()
        ct = ctypes.c_uint32(0xDEAD)
        assert L.psgpu_export_polympus(poly._ctx, None, n, ctypes.byref(ct)) == soa.RET_MPU_VT_OVERFLOW
        assert ct.value == n
        with pytest.raises(gpu.PsgpuError) as e:
            poly.export_polympus()
        assert e.value.code == soa.RET_MPU_VT_OVERFLOW
        stats = np.zeros(n, soa.MPU_STATS_DTYPE)
        rc, got, _ = poly.polygonize_mpus(CS, model, mpus, stats)
        assert (rc, got) == (soa.RET_MPU_VT_OVERFLOW, n) and not mpus.view(np.uint8).any()
        assert poly.finish().firstOverflowMPU == first
        p, m, o = model.ptrs()
        ct = ctypes.c_uint32(0xDEAD)
        assert L.psgpu_polygonize_mpus(poly._ctx, CS, p, m, o, None, n, ctypes.byref(ct), None) == soa.RET_MPU_VT_OVERFLOW
        assert ct.value == n
        # the MPU count is checked first, as the reference checks it
        assert L.psgpu_export_polympus(poly._ctx, mpus.ctypes.data, n - 1, ctypes.byref(ct)) == soa.RET_MPU_OVERFLOW
        _c1_succeeds(lambda cs, mdl, out: poly.polygonize_mpus(cs, mdl, out)[:2])
        assert poly.finish().firstOverflowMPU == -1


def test_polygonize_drop_in_returns_overflow(oracle):
    """gpu.Polygonize (the blocking drop-in on the thread's default context) on zlines: -5 with
    the MPU count, then C1 on the same context: success."""
    du.oracle_mesh(oracle, "zlines")
    mpus = np.zeros(1, soa.MPU_DTYPE)
    rc, ct, _ = gpu.Polygonize(CS, du.model_of("zlines"), mpus)
    assert (rc, ct) == (soa.RET_MPU_VT_OVERFLOW, 1) and not mpus.view(np.uint8).any()
    _c1_succeeds(lambda cs, mdl, out: gpu.Polygonize(cs, mdl, out)[:2])


@pytest.fixture(scope="module")
def group8():
    g = gpu.Group([0] * 8)
    g.set_option(gpu.OPT_JIT, 0)
    g.set_split(list(range(9)))  # one MPU per part
    yield g
    g.close()


@pytest.mark.parametrize("name", [du.RAND_NAMES[0], "mixed"])
def test_group_export_returns_overflow(group8, oracle, name):
    """8 parts over the 8 MPUs: every part reports its own global id, the totals carry the
    smallest across parts (mixed: part 4's), the group export returns -5; C1 afterwards succeeds."""
    L = gpu.load()
    om = du.oracle_mesh(oracle, name)
    flagged = om.stats[:, 4] != 0
    first = int(np.flatnonzero(flagged)[0])
    model = du.model_of(name)
    mpus = np.zeros(8, soa.MPU_DTYPE)
    rc, ct, _ = group8.polygonize_mpus(CS, model, mpus)
    assert (rc, ct) == (soa.RET_MPU_VT_OVERFLOW, 8) and not mpus.view(np.uint8).any()
    total, parts = group8.finish()
    assert total.firstOverflowMPU == first
    assert [p.info.firstOverflowMPU for p in parts] == [m if flagged[m] else -1 for m in range(8)]
    assert [(p.mpuBegin, p.mpuEnd) for p in parts] == [(m, m + 1) for m in range(8)]
    assert (total.ctVertices, total.ctTriangles) == (len(om.pos), len(om.tris))
    st = np.zeros(8, soa.MPU_STATS_DTYPE)
    for k in range(8):
        assert L.psgpu_download_stats(group8.context_ptr(k), st[k:].ctypes.data) == soa.RET_SUCCESS
    assert_mesh_matches(group8.download(), st, om)
    cnt = ctypes.c_uint32()
    assert L.psgpu_group_export_polympus(group8._g, None, 8, ctypes.byref(cnt)) == soa.RET_MPU_VT_OVERFLOW
    # C1 on the same parts (one MPU each of its first 8, the rest on the last part)
    model1, cs1, _ = synth.make_config("C1")
    n1 = gpu.count_mpus(cs1, *model1.bbox)
    group8.set_split(list(range(8)) + [n1])
    try:
        _c1_succeeds(lambda cs, mdl, out: group8.polygonize_mpus(cs, mdl, out)[:2])
        assert group8.finish()[0].firstOverflowMPU == -1
    finally:
        group8.set_split(list(range(9)))


def _export_digests(mpus, stats):
    nv, nt = mpus["ctVertices"].astype(np.int64), mpus["ctTriangles"].astype(np.int64)
    cat = lambda f, n, w: np.concatenate([mpus[f][i, :w * n[i]] for i in range(len(mpus))]).reshape(-1, w)  # noqa: E731
    st4 = np.stack([stats["passedPrecheck"], stats["ctFieldEvals"], stats["ctVertices"], stats["ctTriangles"]], 1)
    return mesh_digests(st4, cat("vPos", nv, 3), cat("vNorm", nv, 3), cat("vColor", nv, 3), cat("triangles", nt, 3))


def test_below_the_limit_exports(poly, group8, oracle):
    """The boundary from below (V up to 321, T up to 494 per MPU, none flagged): the blocking
    export succeeds on a context and on the 8-part group, and PolyMPUs hashes to the oracle's."""
    om = du.oracle_mesh(oracle, "below")
    assert not om.stats[:, 4].any()
    want = mesh_digests(om.stats[:, :4], om.pos, om.nrm, om.col, om.tris)
    model = du.model_of("below")
    with interpreter(poly):
        mpus, stats = np.zeros(8, soa.MPU_DTYPE), np.zeros(8, soa.MPU_STATS_DTYPE)
        rc, ct, _ = poly.polygonize_mpus(CS, model, mpus, stats)
        assert (rc, ct) == (soa.RET_SUCCESS, 8)
        assert poly.finish().firstOverflowMPU == -1
        assert _export_digests(mpus, stats) == want
        gm = np.zeros(8, soa.MPU_DTYPE)
        rc, ct, _ = group8.polygonize_mpus(CS, model, gm)
        assert (rc, ct) == (soa.RET_SUCCESS, 8)
        assert gm.tobytes() == mpus.tobytes()


# ---- 5. the weld ---------------------------------------------------------------------
def test_weld_refuses_an_overflow_run_then_welds_the_next(poly, oracle):
    """A run with an overflow MPU is refused by psgpu_weld (PARAM_ERROR, the published contract),
    psgpu_weld_device / psgpu_download_weld have nothing to give; the next run without one welds
    byte for byte as meshio.weld_lattice on its download."""
    L = gpu.load()
    with interpreter(poly):
        for name in ("checker1x1x2", du.RAND_NAMES[0], "mixed"):
            run_and_compare(poly, oracle, name, runs=1, tag="interp")
            with pytest.raises(gpu.PsgpuError) as e:
                poly.weld()
            assert e.value.code == soa.RET_PARAM_ERROR
            assert L.psgpu_weld(poly._ctx, gpu.PsWeldInfo()) == soa.RET_PARAM_ERROR
            assert L.psgpu_weld_device(poly._ctx, gpu.PsWeldDevice()) == soa.RET_PARAM_ERROR
            assert L.psgpu_download_weld(poly._ctx, None, None, None, None, None) == soa.RET_PARAM_ERROR
        _, om = run_and_compare(poly, oracle, "below", runs=1, tag="interp")
        model = du.model_of("below")
        mesh = poly.download()
        w = poly.weld()
        ref, ref_map = meshio.weld_lattice(mesh, mesh.vertex_offsets, CS, *model.bbox)
        assert w.info.ctInputVertices == len(om.pos) and w.info.ctTriangles == len(om.tris)
        assert (len(w.pos), len(w.tris)) == (w.info.ctVertices, w.info.ctTriangles) == (ref.n_vertices, ref.n_triangles)
        for what, got, exp in (("pos", w.pos, ref.pos), ("nrm", w.nrm, ref.nrm), ("col", w.col, ref.col)):
            assert got.tobytes() == np.ascontiguousarray(exp, np.float32).tobytes(), what
        assert np.array_equal(w.tris, ref.tris.astype(np.uint32))
        assert np.array_equal(w.vertex_map, ref_map.astype(np.uint32))
        assert du.interior_open_edges(w.tris, w.pos, (2, 2, 2))[0] == 0
        assert L.psgpu_weld_device(poly._ctx, gpu.PsWeldDevice()) == soa.RET_SUCCESS


# ---- 6. the field probe -----------------------------------------------------------------
@pytest.mark.parametrize("jit", [0, 1])
def test_checker_field_probe(poly, oracle, jit):
    """field_values (mode 0: the reference's 4-lane groups) at the MPU's 512 corners: the
    oracle's bits, and inside (>= 0.5) exactly where x + y + z is even."""
    x, y, z = (a.reshape(-1).astype(np.float32) for a in np.meshgrid(*[np.arange(8)] * 3, indexing="ij"))
    model = du.model_of("checker")
    try:
        poly.set_option(gpu.OPT_JIT, jit)
        poly.set_model(model)
        assert poly.jit_active == bool(jit)
        f = poly.field_values(np.stack([x, y, z], axis=1) * np.float32(CS), mode=0)
    finally:
        poly.set_option(gpu.OPT_JIT, 1)
    assert_bits_equal(f, oracle.field_value(model, x * np.float32(CS), y * np.float32(CS), z * np.float32(CS)), "field")
    np.testing.assert_array_equal(f >= 0.5, (x + y + z) % 2 == 0)
