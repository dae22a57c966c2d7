"""TEST INFRASTRUCTURE ONLY: ctypes wrapper of the compiled reference (PS::SIMDPOLY itself).

`make -C oracle ref` compiles the reference's PS_Polygonizer.cpp in place from $(PSREF_SRC)
against the serial TBB stand-in (oracle/tbbshim) and oracle/psref_driver.cpp into
oracle/_ref/libpsref.so, and a second build with only MAX_MPU_COUNT raised into
libpsref_big.so (C3's 50,653 MPUs).  Nothing of the reference is part of this repository;
where its source is absent the libraries cannot be built and ``available()`` is False.

Results come back as psoracle.OracleMesh, so the reference, the oracle and the HIP path
compare through the same helpers (tests/parity_util.py).  Only tests/ and
tests/golden/make_reference_goldens.py may use this module.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

from psoracle import OracleMesh

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(HERE, "_ref")
DEFAULT_SRC = "/root/reference/Parsip100/PS_SimdPoly/include"
_SIZES = (9500, 6148, 5636, 21524, 8196)  # prims, prim matrices, ops, MPU, box matrices (parsip_amd/soa.py)
_LIBS = {}
_BUILT = False


def source_dir() -> str:
    return os.environ.get("PSREF_SRC", DEFAULT_SRC)


def source_present() -> bool:
    return os.path.isfile(os.path.join(source_dir(), "PS_Polygonizer.cpp"))


def _path(big: bool) -> str:
    return os.path.join(REF_DIR, "libpsref_big.so" if big else "libpsref.so")


def build() -> None:
    """Run the `ref` target (a no-op without the reference source)."""
    subprocess.run(["make", "-s", "-C", HERE, "ref", f"PSREF_SRC={source_dir()}"], check=True)


def available(big: bool = False) -> bool:
    """True when the reference library exists, building it first where the source is present."""
    global _BUILT
    if not _BUILT and source_present():
        build()
        _BUILT = True
    return os.path.exists(_path(big))


def lib(big: bool = False):
    if big not in _LIBS:
        if not available(big):
            raise RuntimeError(f"{_path(big)} is absent and there is no reference source at {source_dir()}")
        L = ctypes.CDLL(_path(big))
        vp, u32, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
        L.psref_sizes.argtypes = [vp]
        L.psref_polygonize.argtypes = [f32, vp, vp, vp, ctypes.POINTER(vp)]
        L.psref_polygonize.restype = ctypes.c_int
        L.psref_result_info.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(u32)]
        L.psref_result_copy.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.psref_result_free.argtypes = [vp]
        L.psref_prepare_bboxes.argtypes = [f32, vp, vp, vp]
        L.psref_prepare_bboxes.restype = ctypes.c_int
        L.psref_count_mpus.argtypes = [f32, vp, vp]
        L.psref_count_mpus.restype = u32
        L.psref_field_value.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp]
        L.psref_field_value.restype = ctypes.c_int
        L.psref_field_value_and_color.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]
        L.psref_field_value_and_color.restype = ctypes.c_int
        sz = np.zeros(6, np.uint64)
        L.psref_sizes(sz.ctypes.data)
        assert tuple(int(s) for s in sz[:5]) == _SIZES, f"reference struct sizes {sz[:5]} != {_SIZES}"
        L.max_mpus = int(sz[5])
        _LIBS[big] = L
    return _LIBS[big]


def max_mpus(big: bool = False) -> int:
    return lib(big).max_mpus


def polygonize(model, cellsize: float, big: bool = False, origins: bool = False):
    """PS::SIMDPOLY::Polygonize over the whole lattice into a zeroed PolyMPUs -> OracleMesh
    (stats column 0 = ctFieldEvals != 0: the MPU passed the corner precheck).  With
    ``origins=True`` returns (mesh, (ctMPUs, 3) bboxLo)."""
    L = lib(big)
    p, m, o = model.ptrs()
    res = ctypes.c_void_p()
    rc = L.psref_polygonize(cellsize, p, m, o, ctypes.byref(res))
    if rc != 1:
        raise RuntimeError(f"reference Polygonize failed: {rc}")
    try:
        n, v, t = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        L.psref_result_info(res, ctypes.byref(n), ctypes.byref(v), ctypes.byref(t))
        stats = np.zeros((n.value, 5), np.uint32)
        pos = np.zeros((v.value, 3), np.float32)
        nrm = np.zeros_like(pos)
        col = np.zeros_like(pos)
        tri = np.zeros((t.value, 3), np.uint16)
        org = np.zeros((n.value, 3), np.float32)
        L.psref_result_copy(res, stats.ctypes.data, pos.ctypes.data, nrm.ctypes.data, col.ctypes.data,
                            tri.ctypes.data, org.ctypes.data)
    finally:
        L.psref_result_free(res)
    mesh = OracleMesh(0, stats, pos, nrm, col, tri)
    return (mesh, org) if origins else mesh


def _xyz(x, y, z):
    x, y, z = (np.ascontiguousarray(a, np.float32) for a in (x, y, z))
    assert len(x) == len(y) == len(z) and len(x) % 4 == 0
    return x, y, z


def field_value(model, x, y, z) -> np.ndarray:
    """FieldComputer::fieldValue on points grouped 4 at a time (len must be a multiple of 4)."""
    x, y, z = _xyz(x, y, z)
    out = np.zeros(len(x), np.float32)
    p, m, o = model.ptrs()
    rc = lib().psref_field_value(p, m, o, len(x), x.ctypes.data, y.ctypes.data, z.ctypes.data, out.ctypes.data)
    assert rc == 1
    return out


def field_value_and_color(model, x, y, z):
    """FieldComputer::fieldValueAndColor -> (field (n,), colour (n, 3))."""
    x, y, z = _xyz(x, y, z)
    f = np.zeros(len(x), np.float32)
    c = np.zeros((3, len(x)), np.float32)
    p, m, o = model.ptrs()
    rc = lib().psref_field_value_and_color(p, m, o, len(x), x.ctypes.data, y.ctypes.data, z.ctypes.data,
                                           f.ctypes.data, c[0].ctypes.data, c[1].ctypes.data, c[2].ctypes.data)
    assert rc == 1
    return f, c.T.copy()


def count_mpus(cellsize, lo, hi) -> int:
    lo = np.ascontiguousarray(lo, np.float32)
    hi = np.ascontiguousarray(hi, np.float32)
    return int(lib().psref_count_mpus(cellsize, lo.ctypes.data, hi.ctypes.data))


def prepare_bboxes(model, cellsize: float = 0.1) -> int:
    """PrepareBBoxes in place on the model's prims / ops (the cell size is unused by it).
    Every idxMatrix must be below boxmats.count: the reference asserts on that."""
    assert int(model.prims["idxMatrix"][0, :model.ct_prims].max(initial=0)) < max(1, int(model.boxmats["count"][0]))
    return int(lib().psref_prepare_bboxes(cellsize, model.prims.ctypes.data, model.boxmats.ctypes.data,
                                          model.ops.ctypes.data))
