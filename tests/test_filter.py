"""meshio.filter_shells, the host form of psgpu_weld_filter (include/parsip_gpu.h, "the welded
mesh filtered by shell"): hand-made meshes whose answers can be read off, and the CPU oracle's
welds, whose filtered meshes are measured afresh and compared with the kept records.
Thresholds come from tests/golden/shell_counts.json."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from parsip_amd import meshio
from shells_util import cube, fan, golden_counts, two_cubes_interleaved
from test_shells import oracle_shells

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPPED = 0xFFFFFFFF


def attrs(pos):
    """Normals and colours that differ per vertex and from the positions."""
    p = np.asarray(pos, np.float32)
    return p + np.float32(100.0), p * np.float32(0.5) - np.float32(7.0)


def filtered(pos, tris, criteria=None, mask=None):
    nrm, col = attrs(pos)
    sh = meshio.shells(pos, tris)
    return meshio.filter_shells(pos, nrm, col, tris, sh, criteria, mask), sh


def midway(name, field, a, b, absolute=False):
    """Halfway between shells a and b of a golden case in `field`."""
    per = golden_counts()[name]["per_shell"]
    x, y = per[a][field], per[b][field]
    if absolute:
        x, y = abs(x), abs(y)
    assert x != y
    return (x + y) / 2


def test_layout():
    assert meshio.SHELL_FILTER_DTYPE.itemsize == 32 and meshio.SHELL_FILTER_DTYPE.fields["minArea"][1] == 16
    assert meshio.shell_filter().tobytes() == bytes(32)


@pytest.mark.parametrize("mask", [[0, 1], [1, 0]])
def test_interleaved_cubes_by_mask(mask):
    pos, tris = two_cubes_interleaved()
    f, sh = filtered(pos, tris, mask=mask)
    kept = mask.index(1)
    want = np.full(16, DROPPED, np.uint32)
    want[kept::2] = np.arange(8)
    assert f.vertex_map.tolist() == want.tolist()
    assert f.shell_map.tolist() == [DROPPED if m == 0 else 0 for m in mask]
    nrm, col = attrs(pos)
    assert f.pos.tobytes() == pos[kept::2].tobytes() and f.nrm.tobytes() == nrm[kept::2].tobytes()
    assert f.col.tobytes() == col[kept::2].tobytes()
    assert f.tris.dtype == np.uint32 and f.tris.tolist() == ((tris[kept::2] - kept) // 2).tolist()
    assert len(f.shells) == 1 and f.shells["firstVertex"][0] == 0
    rec = f.shells[0].copy()
    rec["firstVertex"] = sh.shells[kept]["firstVertex"]
    assert rec.tobytes() == sh.shells[kept].tobytes()          # no other field changes
    assert meshio.shells(f.pos, f.tris).shells.tobytes() == f.shells.tobytes()   # exact in binary


def cube_with_cavity():
    po, to = cube(4.0)
    pi, ti = cube(2.0)
    return np.concatenate([po, pi]), np.concatenate([to, ti[:, ::-1] + 8])


def test_drop_cavities():
    pos, tris = cube_with_cavity()
    f, sh = filtered(pos, tris, {"flags": meshio.FILTER_DROP_CAVITIES})
    assert sh.shells["volume"].tolist() == [64.0, -8.0] and sh.info["ctClosedShells"] == 2
    assert f.shell_map.tolist() == [0, DROPPED] and f.vertex_map.tolist() == list(range(8)) + [DROPPED] * 8
    assert f.pos.tobytes() == pos[:8].tobytes() and f.tris.tolist() == tris[:12].tolist()
    assert f.shells.tobytes() == sh.shells[:1].tobytes()
    # without the flag the cavity stays; minAbsVolume sees |volume|
    assert filtered(pos, tris, {"minAbsVolume": 8.0})[0].shell_map.tolist() == [0, 1]
    assert filtered(pos, tris, {"minAbsVolume": 8.5})[0].shell_map.tolist() == [0, DROPPED]


def test_closed_only_drops_an_open_cube_and_an_open_cavity_is_no_cavity():
    pa, ta = cube(2.0)
    pb, tb = cube(1.0, (4.0, 0.0, 0.0))
    pos, tris = np.concatenate([pa, pb]), np.concatenate([ta, tb[:-1] + 8])   # cube B lacks a triangle
    f, sh = filtered(pos, tris, {"flags": meshio.FILTER_CLOSED_ONLY})
    assert sh.shells["ctOpenEdges"].tolist() == [0, 3]
    assert f.shell_map.tolist() == [0, DROPPED] and len(f.pos) == 8 and f.tris.tolist() == ta.tolist()
    # DROP_CAVITIES drops closed shells of negative volume only: an open inward-wound cube stays
    pos, tris = cube_with_cavity()
    f, sh = filtered(pos, tris[:-1], {"flags": meshio.FILTER_DROP_CAVITIES})
    assert sh.shells["volume"][1] < 0 and f.shell_map.tolist() == [0, 1]


def test_closed_only_drops_the_fan():
    pos, tris = fan()
    f, sh = filtered(pos, tris, {"flags": meshio.FILTER_CLOSED_ONLY})
    assert sh.shells["ctNonManifoldEdges"].tolist() == [1]
    assert f.shell_map.tolist() == [DROPPED] and f.vertex_map.tolist() == [DROPPED] * 5
    assert f.pos.shape == (0, 3) and f.tris.shape == (0, 3) and len(f.shells) == 0


def test_min_triangles_drops_an_unused_vertex():
    pos, tris = cube()
    pos = np.concatenate([pos[:3], np.float32([[9, 9, 9]]), pos[3:]])   # vertex 3 is in no triangle
    tris = tris + (tris >= 3)
    f, sh = filtered(pos, tris, {"minTriangles": 1})
    assert f.shell_map.tolist() == [0, DROPPED]
    assert f.vertex_map.tolist() == [0, 1, 2, DROPPED, 3, 4, 5, 6, 7]
    assert f.pos.tobytes() == cube()[0].tobytes() and f.tris.tolist() == cube()[1].tolist()
    assert filtered(pos, tris, {"minVertices": 2})[0].tobytes() == f.tobytes()


def test_all_zero_filter_is_the_identity():
    pos, tris = two_cubes_interleaved()
    nrm, col = attrs(pos)
    for criteria in (None, {}, meshio.shell_filter()):
        f, sh = filtered(pos, tris, criteria)
        assert f.vertex_map.tolist() == list(range(16)) and f.shell_map.tolist() == [0, 1]
        assert (f.pos.tobytes(), f.nrm.tobytes(), f.col.tobytes()) == (pos.tobytes(), nrm.tobytes(), col.tobytes())
        assert f.tris.tobytes() == tris.astype(np.uint32).tobytes() and f.shells.tobytes() == sh.shells.tobytes()


def test_keep_nothing_and_an_empty_mesh():
    pos, tris = two_cubes_interleaved()
    f, _ = filtered(pos, tris, mask=[0, 0])
    assert f.vertex_map.tolist() == [DROPPED] * 16 and f.shell_map.tolist() == [DROPPED] * 2
    assert f.pos.shape == f.nrm.shape == f.col.shape == (0, 3) and f.tris.shape == (0, 3) and len(f.shells) == 0
    assert f.tobytes() == b"\xff" * (4 * 18)
    e, _ = filtered(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), {"minTriangles": 5})
    assert e.tobytes() == b"" and e.tris.dtype == np.uint32 and e.vertex_map.dtype == np.uint32


def test_what_the_call_refuses():
    pos, tris = two_cubes_interleaved()
    for bad in ({"flags": 4}, {"reserved": 1}, {"minArea": float("nan")}, {"minArea": -1.0},
                {"minAbsVolume": float("inf")}, {"minVolume": 1.0}):
        with pytest.raises(ValueError):
            filtered(pos, tris, bad)
    with pytest.raises(ValueError):
        filtered(pos, tris, mask=[1])
    sh = meshio.shells(*cube())
    with pytest.raises(ValueError):
        meshio.filter_shells(pos, pos, pos, tris, sh)       # another mesh's shells


def test_argument_rules_of_the_c_abi_under_host_sanitizers(tmp_path):
    """psgpu_weld_filter's argument checks are host code of their own (psgpu_filter_check.h):
    tests/cpp/filter_args_check.cpp, a stand-alone program, runs them under ASan and UBSan."""
    gpp = shutil.which("g++")
    assert gpp is not None, "g++ is needed to compile the argument check"
    exe = tmp_path / "filter_args_check"
    subprocess.run([gpp, "-std=c++17", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "filter_args_check.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr


def split(name, sh):
    """The criteria each oracle case is filtered by (thresholds from the golden counts), and
    the shells that stay."""
    if name == "C2":
        return {"minAbsVolume": midway(name, "volume", 0, 2, absolute=True)}, [True, True, False]
    if name == "cube_minus_point":
        return {"flags": meshio.FILTER_DROP_CAVITIES}, [True, False]
    if name == "rand4_0.123457":
        return {"minTriangles": int(midway(name, "ctTriangles", 0, 1))}, [False, True]
    if name == "rand1_0.13":
        return {"minArea": midway(name, "area", 0, 1)}, [True, False]
    raise KeyError(name)


@pytest.mark.parametrize("name", ["C2", "cube_minus_point", "rand4_0.123457", "rand1_0.13"])
def test_oracle_welds_filtered_and_measured_afresh(oracle, name):
    """meshio.shells of the filtered mesh against the kept records: every integer field and
    bounding box equal; area and volume, whose fixed-point scales differ between the two meshes,
    each within test_shells.py's bound 2 (n + 16) 2^-53 sum|term| of the plain float64 sum of
    the shell's terms (the terms are the same numbers in both meshes)."""
    sh, w = oracle_shells(oracle, name)
    criteria, stays = split(name, sh)
    f = meshio.filter_shells(w.pos, w.nrm, w.col, w.tris, sh, criteria)
    stays = np.array(stays)
    assert (f.shell_map != DROPPED).tolist() == stays.tolist()
    assert f.pos.tobytes() == w.pos[stays[sh.vertex_shell]].tobytes()
    assert f.nrm.tobytes() == w.nrm[stays[sh.vertex_shell]].tobytes()
    assert np.array_equal(f.pos[f.tris], w.pos[w.tris[stays[sh.tri_shell]]])      # the same triangles
    assert (np.diff(f.shells["firstVertex"].astype(np.int64)) > 0).all()
    fresh = meshio.shells(f.pos, f.tris)
    assert len(fresh.shells) == len(f.shells) == int(stays.sum())
    for field in meshio.SHELL_DTYPE.names:
        if field not in ("area", "volume"):
            assert fresh.shells[field].tobytes() == f.shells[field].tobytes(), field
    assert np.array_equal(fresh.vertex_shell, f.shell_map[sh.vertex_shell[stays[sh.vertex_shell]]])
    a2, v6 = meshio.shell_terms(f.pos, f.tris)
    for s in range(len(f.shells)):
        sel = fresh.tri_shell == s
        n = int(sel.sum())
        for field, terms, div in (("area", a2[sel], 2.0), ("volume", v6[sel], 6.0)):
            bound = 2.0 * (n + 16) * 2.0 ** -53 * float(np.abs(terms).sum()) / div
            plain = float(terms.sum()) / div
            print(name, s, field, "kept", float(f.shells[s][field]), "fresh", float(fresh.shells[s][field]),
                  "plain", plain, "bound", bound)
            assert abs(float(f.shells[s][field]) - plain) <= bound
            assert abs(float(fresh.shells[s][field]) - plain) <= bound
    assert meshio.open_edge_count(f.tris) == int(f.shells["ctOpenEdges"].sum())


def test_c2_without_its_sliver(oracle):
    """minAbsVolume between the sliver's and the bodies' |volume|: 2 shells, and exactly the
    sliver's 6 vertices and 8 triangles go."""
    sh, w = oracle_shells(oracle, "C2")
    per = golden_counts()["C2"]["per_shell"]
    sliver = min(range(3), key=lambda s: abs(per[s]["volume"]))
    body = min((s for s in range(3) if s != sliver), key=lambda s: abs(per[s]["volume"]))
    cut = midway("C2", "volume", sliver, body, absolute=True)
    f = meshio.filter_shells(w.pos, w.nrm, w.col, w.tris, sh, {"minAbsVolume": cut})
    assert (per[sliver]["ctVertices"], per[sliver]["ctTriangles"]) == (6, 8)
    assert len(f.shells) == 2 and f.shell_map[sliver] == DROPPED
    assert len(f.pos) == len(w.pos) - 6 and len(f.tris) == len(w.tris) - 8
    first = per[sliver]["firstVertex"]
    assert f.vertex_map[:first].tolist() == list(range(first))      # ids before the sliver stay
    assert int((f.vertex_map == DROPPED).sum()) == 6 and f.vertex_map[-1] == len(w.pos) - 7
