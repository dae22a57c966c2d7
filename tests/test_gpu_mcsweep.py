"""The marching-cubes sweep on the device (tests/mcsweep_util.py): 254 models that put
every cell configuration into every cell position class of an MPU (asserted on the CPU,
tests/test_mcsweep.py), through k_mpu's S3-S6 passes, the weld and the shells.

* every model through the interpreter with default launches: the oracle's mesh bit for bit, one
  vertex record per vertex in the queue, the PolyMPUs export with the oracle's per-MPU counts;
* every 8th model (32, both backgrounds) through each path of test_gpu_cullbound.PATHS with the
  structure-specialised kernels, the baked tier on 4 of them: the launch flags, the same bytes;
* the device weld against meshio.weld_lattice and the device shells against meshio.shells on
  every model, byte for byte; one chunk through a 3-part group, whose seams fall between parts.
"""
import numpy as np
import pytest

import mcsweep_util as mu
from parity_util import assert_mesh_matches
from parsip_amd import gpu, meshio
from test_gpu_cullbound import DEFAULTS, PATHS
from test_gpu_shells import assert_same
from weld_util import check_contract

pytestmark = pytest.mark.gpu

NAMES = mu.names()
CHUNK = 32
CHUNKS = [NAMES[i:i + CHUNK] for i in range(0, len(NAMES), CHUNK)]
CHUNK_IDS = ["%s-%s" % (c[0], c[-1]) for c in CHUNKS]
PATH_NAMES = NAMES[::8]                                  # 21 of the outside background, 11 of the inside one
BAKED_NAMES = [PATH_NAMES[i] for i in (0, 10, 21, 31)]   # the baked tier compiles per model
GROUP_CHUNK = CHUNKS[5]                                  # mc_out160 .. mc_in029: both backgrounds
SPLIT = [0, 3, 6, 8]                                     # the group's parts: MPUs in x-major order
TIER = {"interpreter": 0, "baked": 2}                    # the others run the structure tier (1)
_RUNS = {}


@pytest.fixture(scope="module")
def poly():
    """A context of this module's own at OPT_JIT 0: the interpreter, no compiles."""
    assert gpu.device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"
    p = gpu.Polygonizer(0)
    p.set_option(gpu.OPT_JIT, 0)
    yield p
    p.close()


def mesh_bytes(mesh, stats):
    return tuple(np.ascontiguousarray(a).tobytes() for a in
                 (mesh.pos, mesh.nrm, mesh.col, mesh.tris, mesh.vertex_offsets, mesh.triangle_offsets, stats))


def weld_bytes(w):
    return tuple(np.ascontiguousarray(a).tobytes() for a in (w.pos, w.nrm, w.col, w.tris, w.vertex_map))


class Run:
    """One default-launch interpreter run of a model and everything read back from it."""

    def __init__(self, p, name):
        self.model = mu.model_of(name)
        p.set_model(self.model)
        self.info = p.run(mu.CS)
        self.mesh, self.stats = p.download(), p.stats()
        self.queue = p.vertex_queue()
        self.mpus = p.export_polympus()
        self.weld = p.weld()
        self.shells = p.weld_shells()


def device_run(p, name):
    if name not in _RUNS:
        _RUNS[name] = Run(p, name)
    return _RUNS[name]


@pytest.mark.parametrize("chunk", CHUNKS, ids=CHUNK_IDS)
def test_all_models_match_the_oracle(poly, oracle, chunk):
    for name in chunk:
        r, om = device_run(poly, name), mu.oracle_mesh(oracle, name)
        assert poly.jit_tier == 0 and r.info.ctMPUs == 8, name
        try:
            assert_mesh_matches(r.mesh, r.stats, om)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e
        # the vertex queue: exactly one record (w, r) for every r < V[w] of every MPU w
        counts, shards = r.queue
        recs = np.concatenate(shards).astype(np.int64)
        V = om.stats[:, 2].astype(np.int64)
        want = np.stack([np.repeat(np.arange(len(V)), V), np.concatenate([np.arange(v) for v in V])], axis=1)
        assert int(counts.sum()) == len(want) == r.info.ctVertices, name
        np.testing.assert_array_equal(recs[np.lexsort((recs[:, 1], recs[:, 0]))], want, err_msg=name)
        # the PolyMPUs export: the oracle's per-MPU counts, and its vertices and triangles
        assert len(r.mpus) == len(om.stats), name
        np.testing.assert_array_equal(r.mpus["ctVertices"], om.stats[:, 2], err_msg=name)
        np.testing.assert_array_equal(r.mpus["ctTriangles"], om.stats[:, 3], err_msg=name)
        flat = meshio.from_polympus(r.mpus)
        assert flat.pos.tobytes() == om.pos.tobytes() and np.array_equal(flat.tris, om.global_tris()), name


@pytest.mark.parametrize("path", [p for p in PATHS if p != "baked"] + ["baked"])
def test_paths_give_the_default_runs_bytes(poly, oracle, path):
    opts, must, must_not = PATHS[path]
    names = BAKED_NAMES if path == "baked" else PATH_NAMES
    wants = {name: device_run(poly, name) for name in names}  # the default runs, before the options change
    try:
        for k, v in {**DEFAULTS, **opts}.items():
            poly.set_option(k, v)
        for name in names:
            poly.set_model(mu.model_of(name))
            poly.jit_wait()
            assert poly.jit_tier == TIER.get(path, 1), (name, path, poly.jit_tier)
            info = poly.run(mu.CS)
            mesh, stats = poly.download(), poly.stats()
            assert (info.launchFlags & must) == must and not (info.launchFlags & must_not), (name, path, info.launchFlags)
            try:
                assert_mesh_matches(mesh, stats, mu.oracle_mesh(oracle, name))
            except AssertionError as e:
                raise AssertionError(f"{name} {path}: {e}") from e
            assert mesh_bytes(mesh, stats) == mesh_bytes(wants[name].mesh, wants[name].stats), (name, path)
    finally:
        for k, v in {**DEFAULTS, gpu.OPT_JIT: 0}.items():
            poly.set_option(k, v)


@pytest.mark.parametrize("chunk", CHUNKS, ids=CHUNK_IDS)
def test_weld_and_shells_equal_the_host_forms(poly, chunk):
    for name in chunk:
        r = device_run(poly, name)
        mesh, w = r.mesh, r.weld
        ref, ref_map = meshio.weld_lattice(mesh, mesh.vertex_offsets, mu.CS, *r.model.bbox)
        assert w.info.ctInputVertices == r.info.ctVertices == len(mesh.pos) > 0, name
        assert (len(w.pos), len(w.tris)) == (w.info.ctVertices, w.info.ctTriangles) == (ref.n_vertices, ref.n_triangles), name
        for what, got, want in (("pos", w.pos, ref.pos), ("nrm", w.nrm, ref.nrm), ("col", w.col, ref.col)):
            assert got.tobytes() == np.ascontiguousarray(want, np.float32).tobytes(), (name, what)
        assert np.array_equal(w.tris, ref.tris.astype(np.uint32)), name
        assert np.array_equal(w.vertex_map, ref_map.astype(np.uint32)), name
        check_contract(mesh.pos, mesh.nrm, mesh.col, mesh.tris, w, w.vertex_map)
        _, on_face = mu.seam_classes(mesh, mesh.vertex_offsets, r.model)
        assert w.info.ctSeamVertices == on_face, name
        sh = r.shells
        assert (sh.info["ctVertices"], sh.info["ctTriangles"]) == (w.info.ctVertices, w.info.ctTriangles), name
        assert_same(sh, meshio.shells(w.pos, w.tris))


def test_group_weld_and_shells_equal_the_contexts(poly):
    """One chunk through three parts on one device: the seams fall between parts."""
    g = gpu.Group([0] * 3)
    try:
        g.set_option(gpu.OPT_JIT, 0)
        for name in GROUP_CHUNK:
            want = device_run(poly, name)
            g.set_model(want.model)
            if name == GROUP_CHUNK[0]:
                g.run(mu.CS)
                g.set_split(SPLIT)  # fixed from here on
            g.run(mu.CS)
            assert g.split().tolist() == SPLIT, name
            assert weld_bytes(g.weld()) == weld_bytes(want.weld), name
            assert_same(g.weld_shells(), want.shells)
    finally:
        g.close()
