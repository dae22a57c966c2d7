"""Non-cubic MPU lattices on the CPU (tests/aniso_util.py; the device's side is
tests/test_gpu_aniso.py): the inputs have the properties the device tests rely on, the oracle
equals the compiled reference on them (so it can be the device's reference there too), the host
definitions the device is held to (soa.mpu_origins, the sieve's CPU model, meshio.weld_lattice
through tests/test_weld.py) hold off the cube, and psgpu::div_by is exact at its edges
(tests/cpp/divby_check.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import aniso_util as au
import reference_util as ru
from parity_util import assert_bits_equal
from parsip_amd import soa
from psoracle import OracleMesh
from sieve_util import Sieve
from test_reference import NORMALS_ATOL, ref  # noqa: F401  (the fixture: skips where test_reference.py skips)
from test_sieve import check_dead_bricks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = list(au.LATTICES)
_ID = lambda d: "x".join(str(x) for x in d)  # noqa: E731


def mesh_slice(mesh, begin, end):
    """MPUs [begin, end) of a full-range result, as a run of that range returns them."""
    v, t = mesh.vertex_offsets, mesh.triangle_offsets
    return OracleMesh(begin, mesh.stats[begin:end], mesh.pos[v[begin]:v[end]], mesh.nrm[v[begin]:v[end]],
                      mesh.col[v[begin]:v[end]], mesh.tris[t[begin]:t[end]])


# ---- what the tests ask of their inputs ------------------------------------------------------
def test_lattice_set():
    """Every named lattice has three pairwise distinct dims or contains a 1, and comes with its
    two cyclic rotations."""
    for d in DIMS:
        assert len(set(d)) == 3 or 1 in d, d
        assert d[1:] + d[:1] in au.LATTICES and d[2:] + d[:2] in au.LATTICES, d
    assert len(DIMS) >= 12


@pytest.mark.parametrize("dims", DIMS, ids=_ID)
def test_named_lattice_has_a_mesh_along_every_axis(oracle, dims):
    model, cs = au.lattice_case(dims)
    om = oracle.polygonize(model, cs, threads=4)
    assert len(om.stats) == int(np.prod(dims))
    assert len(om.pos) >= 150, len(om.pos)
    surf = np.flatnonzero(om.stats[:, 2] > 0)
    ijk = np.stack(np.unravel_index(surf, dims), axis=1)
    for a in range(3):
        if dims[a] >= 2:
            assert len(set(ijk[:, a])) >= 2, (dims, a)


@pytest.mark.parametrize("dims", DIMS, ids=_ID)
def test_named_ranges_are_ragged(dims):
    d0, d1, d2 = dims
    nyz, n = d1 * d2, d0 * d1 * d2
    r = au.RANGES[dims]
    assert r["full"] == (0, n) and r["first"] == (0, 1) and r["last"] == (n - 1, n)
    for b, e in r.values():
        assert 0 <= b < e <= n
    b, e = r["ragged"]
    if d0 > 1:
        assert (b // nyz) % 2 == 1  # an odd x-row: the brick row starts one MPU row before it
    if d2 > 1:
        assert b % d2 != 0 and e % d2 != 0  # mid z-row at both ends
    if nyz > 2:
        assert b % nyz != 0 and e % nyz != 0
    b, e = r["in_row"]
    assert b // nyz == (e - 1) // nyz


def test_sieve_model_has_both_outcomes():
    both = 0
    for d in DIMS:
        model, cs = au.lattice_case(d)
        sv = Sieve(model, cs, "aniso_both_" + _ID(d))
        assert sv.valid == 1 and sv.dead.shape == tuple((x + 1) // 2 for x in d)
        both += bool(sv.dead.any() and not sv.dead.all())
    assert both >= 8, both


def test_fuzz_boxes(oracle):
    empty = 0
    for s in range(40):
        model, cs, b, e, _, _, _ = au.fuzz_box_case(s)
        d = soa.mpu_dims(cs, *model.bbox)
        assert len(set(d)) == 3, (s, d)
        assert 0 <= b < e <= int(np.prod(d))
        empty += int(oracle.polygonize(model, cs, b, e, threads=4, keep=False).stats[:, 2].sum()) == 0
    assert empty <= 8, empty


# ---- the oracle against the compiled reference -----------------------------------------------
def _against_reference(ref, oracle, model, cs, rng, what):  # noqa: F811
    """The SSE build bit for bit, and on trees without Disc / Ring / RicciBlend the IEEE build
    with normals within NORMALS_ATOL: the full range, and the range ``rng`` against those MPUs
    of the reference's (full-range) result."""
    r, org = ref.polygonize(model, cs, origins=True)
    for sse in (True,) if ru.has_approx(model) else (True, False):
        atol = None if sse else NORMALS_ATOL
        ru.assert_oracle_mesh_equal(oracle.polygonize(model, cs, threads=4, sse_approx=sse), r, what, normals_atol=atol)
        ru.assert_oracle_mesh_equal(oracle.polygonize(model, cs, *rng, threads=4, sse_approx=sse),
                                    mesh_slice(r, *rng), f"{what} MPUs {rng}", normals_atol=atol)
    return r, org


@pytest.mark.parametrize("dims", DIMS, ids=_ID)
def test_oracle_equals_reference_on_named_lattices(ref, oracle, dims):  # noqa: F811
    model, cs = au.lattice_case(dims)
    assert not ru.has_approx(model)
    r, org = _against_reference(ref, oracle, model, cs, au.RANGES[dims]["ragged"], _ID(dims))
    n = int(np.prod(dims))
    assert len(r.stats) == n == ref.count_mpus(cs, *model.bbox) == oracle.count_mpus(cs, *model.bbox) == \
        soa.count_mpus(cs, *model.bbox)
    # the reference's per-MPU bboxLo: what soa.mpu_origins (and through it the drop-in
    # Polygonize and meshio.weld_lattice) says, whole and from the middle of a row
    assert_bits_equal(soa.mpu_origins(cs, *model.bbox), org, "MPU origins")
    b, e = au.RANGES[dims]["ragged"]
    assert_bits_equal(soa.mpu_origins(cs, *model.bbox, b, e), org[b:e], "MPU origins of a range")


@pytest.mark.parametrize("seed", range(40))
def test_oracle_equals_reference_on_fuzz_boxes(ref, oracle, seed):  # noqa: F811
    model, cs, b, e, _, _, _ = au.fuzz_box_case(seed)
    _, org = _against_reference(ref, oracle, model, cs, (b, e), f"seed {seed}")
    assert_bits_equal(soa.mpu_origins(cs, *model.bbox), org, "MPU origins")


# ---- the sieve's CPU model -------------------------------------------------------------------
@pytest.mark.parametrize("dims", DIMS, ids=_ID)
def test_dead_bricks_on_named_lattices(oracle, dims):
    """No S1 survivor in a dead brick, on every range; and Sieve.live_set (what the device's
    live list is compared with) against a list built here brick by brick."""
    model, cs = au.lattice_case(dims)
    for name, (b, e) in au.RANGES[dims].items():
        sv, _, _ = check_dead_bricks(oracle, f"aniso_{_ID(dims)}_{name}", model, cs, b, e)
        assert sv.valid == 1 and sv.dims == tuple(dims)
        want = set()
        for bi in range(sv.nb[0]):
            for bj in range(sv.nb[1]):
                for bk in range(sv.nb[2]):
                    ids = [((2 * bi + x) * dims[1] + 2 * bj + y) * dims[2] + 2 * bk + z
                           for x in (0, 1) for y in (0, 1) for z in (0, 1)
                           if 2 * bi + x < dims[0] and 2 * bj + y < dims[1] and 2 * bk + z < dims[2]]
                    if not sv.dead[bi, bj, bk] and any(b <= m < e for m in ids):
                        want.add((bi, bj, bk))
        assert sv.live_set(b, e) == want, name


# ---- div_by ----------------------------------------------------------------------------------
def test_div_by_is_exact(tmp_path):
    """tests/cpp/divby_check.cpp: every d in 1..4096 and six wide ones at their edge values and
    10^5 random ones each; the MPU and brick decodes of every named lattice, which must also be
    numpy's unravel_index."""
    gpp = shutil.which("g++")
    assert gpp is not None, "g++ is needed to compile tests/cpp/divby_check.cpp"
    exe, out = tmp_path / "divby_check", tmp_path / "decode.bin"
    subprocess.run([gpp, "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "parsip_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "divby_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(out)] + [str(x) for d in DIMS for x in d], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    bricks = [tuple((x + 1) // 2 for x in d) for d in DIMS]
    per_d = 9 + 100000  # edge values and random ones; k * d - 1 and k * d come on top
    assert int(r.stdout.split()[0]) >= 4102 * per_d + sum(int(np.prod(d)) + int(np.prod(b)) for d, b in zip(DIMS, bricks))
    got = np.fromfile(out, np.uint32).reshape(-1, 3)
    want = np.concatenate([np.stack(np.unravel_index(np.arange(int(np.prod(s))), s), axis=1)
                           for d, b in zip(DIMS, bricks) for s in (d, b)])
    np.testing.assert_array_equal(got, want)
