"""bench.py's roofline reads the committed PMC / traffic summaries of the kernel tier it timed
(verdict r03: the baked tier's counters must never price a structure-tier step).  CPU only:
the selection logic over synthetic profile files."""
import importlib.util
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def bench(tmp_path, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "4")  # bench sets it at import: restored after the test
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # no HIP call at import
    (tmp_path / "profiles").mkdir()
    monkeypatch.setattr(mod, "ROOT", str(tmp_path))
    return mod


def _write(tmp_path, name, jit, instr):
    d = {"kernels": {"jit_mpu": {"SQ_INSTS_VALU": instr, "launches": 1}}}
    if jit is not None:
        d["jit"] = jit
    (tmp_path / "profiles" / name).write_text(json.dumps(d))


def test_profile_of_the_timed_tier(bench, tmp_path):
    _write(tmp_path, "r03_pmc.json", None, 1.0)       # before r04: no "jit", profiled with --jit 2
    _write(tmp_path, "r04_pmc.json", 2, 2.0)
    _write(tmp_path, "r04_pmc_structure.json", 1, 3.0)
    k, src = bench.committed_profile("pmc", 2)
    assert src.endswith("r04_pmc.json") and k["jit_mpu"]["SQ_INSTS_VALU"] == 2.0
    k, src = bench.committed_profile("pmc_structure", 1)
    assert src.endswith("r04_pmc_structure.json") and k["jit_mpu"]["SQ_INSTS_VALU"] == 3.0
    # a file whose recorded tier differs is never used for another tier
    assert bench.committed_profile("pmc", 1) == (None, None)
    assert bench.committed_profile("pmc_structure", 2) == (None, None)


def test_old_profiles_count_as_baked(bench, tmp_path):
    _write(tmp_path, "r03_pmc.json", None, 1.0)
    k, src = bench.committed_profile("pmc", 2)
    assert src.endswith("r03_pmc.json")
    assert bench.committed_profile("pmc", 1) == (None, None)


def test_profile_entry_names(bench):
    kernels = {"jit_mpu": {"a": 1}, "psgpu::k_mpu": {"a": 2}}
    assert bench.profile_entry(kernels, "k_mpu", 1) == {"a": 1}
    assert bench.profile_entry(kernels, "k_mpu", 0) == {"a": 2}
    assert bench.profile_entry(None, "k_mpu", 1) is None


def test_dump_outputs_sample_is_seeded(bench, tmp_path):
    """--dump-outputs: a mesh past the byte budget is cut to the same seeded rows of every
    array, in the mesh's order, and two dumps of it are identical."""
    import numpy as np

    from parsip_amd import gpu

    V, T = 1000, 1500
    f = np.arange(V * 3, dtype=np.float32).reshape(V, 3)
    mesh = gpu.Mesh(f, f + 0.5, f + 0.25, np.arange(T * 3, dtype=np.uint32).reshape(T, 3),
                    np.arange(11, dtype=np.int64), np.arange(11, dtype=np.int64) * 2)
    names = ("pos", "nrm", "col", "vertex_nonfinite", "tris", "vertex_offsets", "triangle_offsets")
    whole = 6 * f.nbytes + T * 3 * 8 + 2 * 11 * 8
    a, b, c = (str(tmp_path / d) for d in "abc")
    bench.dump_outputs(a, mesh, budget=whole // 4)
    bench.dump_outputs(b, mesh, budget=whole // 4)
    size = 0
    for n in names:
        x, y = np.load(os.path.join(a, n + ".npy")), np.load(os.path.join(b, n + ".npy"))
        assert x.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(x, y)
        size += x.nbytes
    assert 0 < size <= whole // 4
    pos, nrm = np.load(os.path.join(a, "pos.npy")), np.load(os.path.join(a, "nrm.npy"))
    assert len(pos) == V // 4 and np.all(np.diff(pos[:, 0]) > 0)
    np.testing.assert_array_equal(nrm, pos + 0.5)
    # within the budget nothing is cut
    bench.dump_outputs(c, mesh, budget=whole)
    np.testing.assert_array_equal(np.load(os.path.join(c, "tris.npy")), mesh.tris)
    np.testing.assert_array_equal(np.load(os.path.join(c, "col.npy")), mesh.col)
    nf = np.load(os.path.join(c, "vertex_nonfinite.npy"))
    assert nf.shape == (V, 9) and nf.dtype == np.float32 and not nf.any()
    assert np.load(os.path.join(a, "vertex_nonfinite.npy")).shape == (V // 4, 9)  # the rows of pos


def test_dump_outputs_files_are_finite(bench, tmp_path):
    """A non-finite element (the reference's NaN normal at a zero gradient) is written as 0
    and its kind marked in vertex_nonfinite.npy, whose shape the values do not change; the
    rest is untouched."""
    import numpy as np

    from parsip_amd import gpu

    V = 7
    f = np.arange(V * 3, dtype=np.float32).reshape(V, 3) + 1
    nrm = f.copy()
    nrm[2] = np.nan
    nrm[5, 0], nrm[5, 2] = np.inf, -np.inf
    mesh = gpu.Mesh(f, nrm, f, np.zeros((2, 3), np.uint32), np.arange(3, dtype=np.int64), np.arange(3, dtype=np.int64))
    info = bench.dump_outputs(str(tmp_path / "d"), mesh)
    got = np.load(tmp_path / "d" / "nrm.npy")
    nf = np.load(tmp_path / "d" / "vertex_nonfinite.npy")
    assert got.dtype == np.float32 and np.isfinite(got).all() and nf.dtype == np.float32
    marks = np.zeros((V, 9), np.float32)
    marks[2, 3:6] = 1
    marks[5, 3], marks[5, 5] = 2, 3
    np.testing.assert_array_equal(nf, marks)
    want = f.copy()
    want.reshape(-1)[[6, 7, 8, 15, 17]] = 0
    np.testing.assert_array_equal(got, want)
    assert info["nrm"]["nonfinite"] == 5 and info["pos"]["nonfinite"] == 0
    assert np.isnan(mesh.nrm[2]).all()  # the caller's mesh is not modified
