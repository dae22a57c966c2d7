"""The marching-cubes sweep on the CPU (tests/mcsweep_util.py): its 254 models put
every cell configuration into every cell position class of an MPU, which is asserted here from
the oracle's own field values; they stay within what every kernel path and the export take; their
seams cover every crossing-edge axis and multiplicity; the oracle's two builds, the compiled
reference and the committed digests agree on them; the host weld closes them; and the packed
tables k_mpu's record passes read are what a naive derivation from the triangle table gives
(tests/cpp/mctables_check.cpp).  tests/test_gpu_mcsweep.py runs the HIP path on the same models."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import mcsweep_util as mu
from dense_util import interior_open_edges
from parity_util import assert_bits_equal
from parsip_amd import meshio, soa
from reference_util import assert_oracle_mesh_equal
from weld_util import check_contract

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMALS_ATOL = 2e-3  # as test_dense.py::test_sse_and_ieee_builds_agree


@pytest.fixture(scope="module")
def sweep(oracle):
    """[(name, model, IEEE oracle mesh)] of every model (the meshes are shared and read-only)."""
    return [(name, model, mu.oracle_mesh(oracle, name)) for name, model in mu.models()]


@pytest.fixture(scope="module")
def ref(oracle):
    import psref

    if not psref.source_present() and not os.path.exists(os.path.join(psref.REF_DIR, "libpsref.so")):
        pytest.skip(f"no compiled reference in oracle/_ref and no reference source at {psref.source_dir()}")
    assert psref.available()
    return psref


def test_every_configuration_in_every_position_class(oracle, sweep):
    """All 254 x 27 (configuration, position class) pairs occur in MPUs the oracle polygonized,
    and so do the 254 x 8 pairs of the ownership projection that selects CubeTablesDev::own."""
    hist = np.zeros((256, 27), np.int64)
    for _, model, _ in sweep:
        hist += mu.coverage(oracle, model)
    covered = int((hist[1:255] > 0).sum())
    own = int((mu.own_projection(hist)[1:255] > 0).sum())
    print(f"{len(sweep)} models: {covered} of 6,858 pairs, {own} of 2,032 ownership pairs, "
          f"{int(hist[1:255].sum())} surface cells")
    missing = np.argwhere(hist[1:255] == 0)
    assert covered == 254 * 27, missing[:10] + [1, 0]
    assert own == 254 * 8


def test_the_sites_hold_what_was_written(oracle):
    """The construction itself, on the first and last model of each background: every site's
    cell has exactly the configuration written into it."""
    for bg in mu.BACKGROUNDS:
        for m in (0, len(mu.configs(bg)) - 1):
            model = mu.model_of("mc_%s%03d" % (bg, m))
            cfg = mu.mpu_configs(oracle, model).reshape(2, 2, 2, 7, 7, 7)
            for (gx, gy, gz), want in mu.sites(bg, m):
                assert cfg[gx // 7, gy // 7, gz // 7, gx % 7, gy % 7, gz % 7] == want, (bg, m, (gx, gy, gz))


def test_conditions_per_model(sweep):
    """Every model stays inside what all kernel paths and the PolyMPUs export take, and the
    whole set has two tree structures (one compile of the specialised kernels each)."""
    failed_s1 = mpus = max_v = max_t = 0
    for name, model, om in sweep:
        assert not om.stats[:, 4].any(), name
        assert om.stats[:, 2].max() <= soa.MAX_MPU_VERTEX_COUNT and om.stats[:, 3].max() <= soa.MAX_MPU_TRIANGLE_COUNT, name
        assert not np.isnan(om.pos).any() and not np.isnan(om.nrm).any(), name
        assert model.ct_prims <= 128 and model.ct_ops <= 128, name
        assert len(om.stats) == 8 and int(om.stats[:, 3].sum()) > 0, name
        failed_s1 += int((om.stats[:, 0] == 0).sum())
        mpus += len(om.stats)
        max_v, max_t = max(max_v, int(om.stats[:, 2].max())), max(max_t, int(om.stats[:, 3].max()))
    print(f"max V {max_v}, max T {max_t} per MPU; {failed_s1} of {mpus} MPUs fail S1")
    assert failed_s1 <= 0.02 * mpus
    assert len({mu.structure(model) for _, model, _ in sweep}) <= 2
    assert len(sweep) == 254 and len({name for name, _, _ in sweep}) == 254


def test_inside_background_takes_the_tree_split(sweep):
    """The root of the inside background has two operator children (OPT_TREE_SPLIT's condition),
    and so has the outside background's."""
    for _, model, _ in sweep:
        assert int(model.ops["opChildKind"][0, 0]) == 3


def test_seams_cover_every_axis_and_multiplicity(sweep):
    """Among the input vertices there is, for each axis, a crossing edge inside an MPU, one on a
    face between two MPUs (2 copies) and one on the line where four MPUs meet (4 copies)."""
    seen = {}
    for name, model, om in sweep:
        classes, _ = mu.seam_classes(meshio.TriMesh(om.pos, om.global_tris()), om.vertex_offsets, model)
        for c in classes:
            seen[c] = seen.get(c, 0) + 1
    print("models per (axis, copies):", sorted(seen.items()))
    assert set(seen) == {(a, n) for a in range(3) for n in (1, 2, 4)}


def test_sse_and_ieee_builds_agree(oracle, sweep):
    """UNION / DIF over POINTs and a CUBE: no Disc, Ring or RicciBlend, so stats, positions,
    triangles and colours are the same bits and the normals differ by the rsqrt alone."""
    for name, model, a in sweep:
        b = mu.oracle_mesh(oracle, name, sse_approx=True)
        np.testing.assert_array_equal(a.stats, b.stats, err_msg=name)
        assert_bits_equal(a.pos, b.pos, f"{name}: positions")
        np.testing.assert_array_equal(a.tris, b.tris, err_msg=name)
        assert_bits_equal(a.col, b.col, f"{name}: colours")
        assert np.abs(a.nrm - b.nrm).max() <= NORMALS_ATOL, name


def test_sse_oracle_equals_reference(ref, oracle, sweep):
    for name, model, _ in sweep:
        assert_oracle_mesh_equal(mu.oracle_mesh(oracle, name, sse_approx=True), ref.polygonize(model, mu.CS), name)


def test_oracle_digests_match_golden(sweep):
    with open(mu.GOLDEN) as f:
        gold = json.load(f)["models"]
    assert list(gold) == [name for name, _, _ in sweep]
    for name, _, om in sweep:
        assert mu.digest(om) == gold[name], name


def test_host_weld_closes_every_inner_seam(sweep):
    """meshio.weld_lattice on every oracle mesh: the weld's contract holds and no edge used by
    one triangle only lies inside the box; meshio.shells counts the same open edges."""
    merged = 0
    for name, model, om in sweep:
        tris = om.global_tris()
        w, vmap = meshio.weld_lattice(meshio.TriMesh(om.pos, tris, om.nrm, om.col), om.vertex_offsets, mu.CS, *model.bbox)
        check_contract(om.pos, om.nrm, om.col, tris, w, vmap)
        assert w.n_triangles == len(om.tris), name
        merged += len(om.pos) - w.n_vertices
        inner, total = interior_open_edges(w.tris, w.pos, mu.DIMS)
        assert inner == 0, (name, inner, total)
        assert total == meshio.open_edge_count(w.tris), name
        sh = meshio.shells(w.pos, w.tris)
        assert int(sh.info["ctOpenEdges"]) == total, name
        assert int(sh.info["ctTriangles"]) == w.n_triangles and int(sh.info["ctVertices"]) == w.n_vertices, name
    assert merged > 0


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_derived_tables(oracle, tmp_path, sanitize):
    """tests/cpp/mctables_check.cpp: cube_tables / fill_device_tables (psgpu_model.h) as plain
    g++ code against the oracle's triangle table: all 256 x 8 (configuration, ownership class)
    counts, every k-th owned edge, all 343 x 12 CellEdge slots; once more under AddressSanitizer
    and UBSan (a program of its own: nothing is preloaded)."""
    gpp = shutil.which("g++")
    assert gpp is not None, "g++ is needed to compile tests/cpp/mctables_check.cpp"
    exe, src = tmp_path / "mctables_check", tmp_path / "tritable.bin"
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.run([gpp, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I",
                    os.path.join(ROOT, "parsip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "mctables_check.cpp"), "-o", str(exe)], check=True)
    oracle.tritable().astype("<i4").tofile(src)
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    got = dict(zip(words[::2], (int(x) for x in words[1::2])))
    # owned crossing edges over all pairs: an edge crosses in 128 configurations and is owned in
    # 8, 4, 4 or 2 of the 8 classes (by how many of its off-axis coordinates are low), per axis
    assert got == {"configs": 256, "own_pairs": 256 * 8, "kth_edges": 128 * 3 * (8 + 4 + 4 + 2),
                   "cell_edges": 343 * 12, "failures": 0}
