"""Mesh output for the polygonizer's result.

The reference consumes `PolyMPUs` per MPU (SimdPoly::draw,
Parsip100/ParsipHaptics/include/PS_HighPerformanceRender.cpp:378-426: one GL vertex /
normal / colour array and one U16 index list per MPU with ctTriangles > 0) and saves
meshes through CMeshVV::save (Parsip100/PS_FrameWork/include/PS_MeshVV.cpp:1023-1163:
OFF and ASCII PLY with "property float32 x|y|z" and "property list uint8 int32
vertex_indices", written in stream order).  Here:

* `from_polympus` turns the reference PolyMPUs layout (e.g. from
  `gpu.Polygonizer.export_polympus`) into one compact mesh, MPU by MPU, as draw() walks it;
* `weld` merges the duplicate vertices MPUs emit on shared faces (exact position bits;
  the reference keeps them, since every MPU is drawn on its own);
* `weld_lattice` merges them by the lattice edge each vertex sits on instead (exact for every
  cell size: neighbouring MPUs round a shared corner differently, DESIGN.md §6 "Weld"); the
  device form is `gpu.Polygonizer.weld`;
* `weld_by_edges` is that weld for edges the caller names (the compat mode's mesh, whose
  positions do not tell them: `gui.lattice_edges`);
* `write_off`, `write_ply` follow CMeshVV::save's text layouts; `write_obj` adds the
  common OBJ form with normals (v / vn / f a//a b//b c//c).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import soa


@dataclass
class TriMesh:
    pos: np.ndarray          # (V, 3) f32
    tris: np.ndarray         # (T, 3) integer vertex ids
    nrm: np.ndarray | None = None
    col: np.ndarray | None = None

    @property
    def n_vertices(self) -> int:
        return len(self.pos)

    @property
    def n_triangles(self) -> int:
        return len(self.tris)


def from_mesh(mesh) -> TriMesh:
    """A gpu.Mesh (compact device download) as a TriMesh (global u32 ids)."""
    return TriMesh(mesh.pos, mesh.tris.astype(np.int64), mesh.nrm, mesh.col)


def from_polympus(mpus: np.ndarray, ct_mpus: int | None = None) -> TriMesh:
    """Concatenate vMPUs[0..ctMPUs) (soa.MPU_DTYPE) in draw() order."""
    n = len(mpus) if ct_mpus is None else ct_mpus
    pos, nrm, col, tris = [], [], [], []
    base = 0
    for i in range(n):
        m = mpus[i]
        nv, nt = int(m["ctVertices"]), int(m["ctTriangles"])
        if nt == 0:
            continue
        pos.append(m["vPos"][:nv * 3].reshape(-1, 3))
        nrm.append(m["vNorm"][:nv * 3].reshape(-1, 3))
        col.append(m["vColor"][:nv * 3].reshape(-1, 3))
        tris.append(m["triangles"][:nt * 3].reshape(-1, 3).astype(np.int64) + base)
        base += nv
    if not pos:
        z = np.zeros((0, 3), np.float32)
        return TriMesh(z, np.zeros((0, 3), np.int64), z, z)
    return TriMesh(np.concatenate(pos), np.concatenate(tris), np.concatenate(nrm), np.concatenate(col))


def weld(mesh: TriMesh) -> TriMesh:
    """Merge vertices with bit-identical positions (first occurrence keeps its normal and
    colour); drops triangles that become degenerate."""
    if mesh.n_vertices == 0:
        return mesh
    key = np.ascontiguousarray(mesh.pos, np.float32).view(np.uint32).reshape(-1, 3)
    _, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)
    remap = np.empty_like(order)
    remap[order] = np.arange(len(order))
    new_id = remap[inverse.reshape(-1)]
    keep = first[order]
    tris = new_id[mesh.tris]
    ok = (tris[:, 0] != tris[:, 1]) & (tris[:, 1] != tris[:, 2]) & (tris[:, 0] != tris[:, 2])
    return TriMesh(mesh.pos[keep], tris[ok], None if mesh.nrm is None else mesh.nrm[keep],
                   None if mesh.col is None else mesh.col[keep])


def lattice_edges(mesh, vertex_offsets, cellsize: float, lo, hi, mpu_begin: int = 0) -> np.ndarray:
    """The global lattice edge (gx, gy, gz, axis) of every vertex of a concatenation of per-MPU
    meshes (arguments as `weld_lattice`), (V, 4) int64, recovered from the positions: a vertex
    of MPU (i, j, k) on the edge from corner (sx, sy, sz) along `axis` has
    g = (7i + sx, 7j + sy, 7k + sz).  Its two off-axis coordinates equal
    ``origin + cellsize * float(s)`` of its MPU bit for bit for some s in 0..7, the third lies
    in cell [s, s + 1) of the axis.  ValueError on a vertex with fewer than two such
    coordinates, and on one with three (a root exactly on a lattice corner: its axis cannot
    be told from positions alone).  A vertex is on an MPU face iff an off-axis g is a multiple
    of 7."""
    pos = np.ascontiguousarray(mesh.pos, np.float32).reshape(-1, 3)
    voff = np.asarray(vertex_offsets, np.int64)
    n, V = len(voff) - 1, len(pos)
    if voff[-1] != V:
        raise ValueError(f"vertex_offsets end at {int(voff[-1])}, the mesh has {V} vertices")
    if V == 0:
        return np.zeros((0, 4), np.int64)
    dims = soa.mpu_dims(cellsize, lo, hi)
    w = np.repeat(np.arange(n, dtype=np.int64), np.diff(voff))
    org = soa.mpu_origins(cellsize, lo, hi, mpu_begin, mpu_begin + n)[w]
    m = w + mpu_begin
    ijk = (m // (dims[2] * dims[1]), (m // dims[2]) % dims[1], m % dims[2])
    cs = np.float32(cellsize)
    steps = cs * np.arange(8, dtype=np.float32)            # cs * (float)s, one rounding
    exact = np.zeros((V, 3), bool)
    s = np.zeros((V, 3), np.int64)
    cell = np.zeros((V, 3), np.int64)
    inside = np.zeros((V, 3), bool)
    for a in range(3):
        corner = org[:, a, None] + steps[None, :]          # (V, 8) f32: origin + cs * s
        hit = corner.view(np.uint32) == pos[:, a].view(np.uint32)[:, None]
        exact[:, a] = hit.any(axis=1)
        s[:, a] = hit.argmax(axis=1)
        cell[:, a] = np.minimum((corner[:, 1:] <= pos[:, a, None]).sum(axis=1), 6)
        inside[:, a] = (pos[:, a] >= corner[:, 0]) & (pos[:, a] <= corner[:, 7])
    ct = exact.sum(axis=1)
    if (ct < 2).any():
        v = int(np.flatnonzero(ct < 2)[0])
        raise ValueError(f"vertex {v} {pos[v]} is not on a lattice edge of its MPU")
    if (ct > 2).any():
        v = int(np.flatnonzero(ct > 2)[0])
        raise ValueError(f"{int((ct > 2).sum())} vertices are exactly on a lattice corner (first: vertex {v} "
                         f"{pos[v]}): their edges are ambiguous")
    axis = (~exact).argmax(axis=1)
    rows = np.arange(V)
    if not inside[rows, axis].all():
        v = int(np.flatnonzero(~inside[rows, axis])[0])
        raise ValueError(f"vertex {v} {pos[v]} is outside its MPU")
    s[rows, axis] = cell[rows, axis]
    return np.stack([7 * ijk[0] + s[:, 0], 7 * ijk[1] + s[:, 1], 7 * ijk[2] + s[:, 2], axis], axis=1)


def weld_lattice(mesh, vertex_offsets, cellsize: float, lo, hi, mpu_begin: int = 0):
    """Merge the vertices MPUs emit on shared faces by lattice-edge identity; returns
    ``(TriMesh, vertex_map)``.

    ``mesh`` is the concatenation of per-MPU meshes of MPUs ``[mpu_begin, mpu_begin + n)`` of the
    lattice of ``cellsize`` over the box ``lo``..``hi`` (a ``gpu.Mesh`` download, or a TriMesh
    with global ids), ``vertex_offsets`` its ``n + 1`` per-MPU vertex offsets.  Vertices on the
    same lattice edge (`lattice_edges`, which raises ValueError on a vertex whose edge the
    positions do not determine) are one welded vertex, welded vertices are ordered by their
    first occurrence and take its position, normal and colour, ``vertex_map[v]`` is the welded
    id of input vertex v and the triangles are ``vertex_map[mesh.tris]`` (none drops: an MPU has
    one vertex per edge).  Seams towards MPUs outside the range stay open.  The device form is
    ``gpu.Polygonizer.weld`` (same bytes)."""
    g = lattice_edges(mesh, vertex_offsets, cellsize, lo, hi, mpu_begin)
    if len(g) and max(soa.mpu_dims(cellsize, lo, hi)) * 7 >= 1 << 20:  # the device's limit too (psgpu_weld)
        raise ValueError("lattice too large for the edge key")
    return weld_by_edges(mesh, g)


def weld_by_edges(mesh, edges):
    """Merge the vertices with equal lattice edges; returns ``(TriMesh, vertex_map)``.

    ``edges`` names the global lattice edge (gx, gy, gz, axis) of every vertex of ``mesh``,
    (V, 4) (`lattice_edges` for a hot-path mesh, ``gui.lattice_edges`` or
    ``gui.ParsipOptimized.vertex_edges()`` for a compat mesh).  Welded vertices are ordered by
    their first occurrence and take its position, normal and colour (of any width) bit for bit,
    ``vertex_map[v]`` is the welded id of input vertex v, the triangles are
    ``vertex_map[mesh.tris]`` and none drops.  It is the weld inside `weld_lattice`, and the
    host form of ``gui.ParsipOptimized.weld`` (same bytes)."""
    pos = np.ascontiguousarray(mesh.pos, np.float32).reshape(-1, 3)
    tris_in = np.asarray(mesh.tris).astype(np.int64)
    g = np.asarray(edges).astype(np.int64).reshape(-1, 4)
    if len(g) != len(pos):
        raise ValueError(f"{len(g)} edges for {len(pos)} vertices")
    if len(pos) == 0:
        return TriMesh(pos, tris_in, mesh.nrm, mesh.col), np.zeros(0, np.int64)
    if g.min() < 0 or g[:, :3].max() >= 1 << 20 or g[:, 3].max() > 2:
        raise ValueError("an edge does not fit the edge key (20 bits a coordinate, axis 0..2)")
    key = (((g[:, 0] << 20 | g[:, 1]) << 20 | g[:, 2]) << 2) | g[:, 3]
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first)
    remap = np.empty_like(order)
    remap[order] = np.arange(len(order))
    vertex_map = remap[inverse.reshape(-1)]
    keep = first[order]
    return (TriMesh(pos[keep], vertex_map[tris_in], None if mesh.nrm is None else np.asarray(mesh.nrm)[keep],
                    None if mesh.col is None else np.asarray(mesh.col)[keep]), vertex_map)


def open_edge_count(tris) -> int:
    """Undirected edges used by exactly one triangle (0 on a closed surface)."""
    t = np.asarray(tris).astype(np.int64).reshape(-1, 3)
    if len(t) == 0:
        return 0
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    e.sort(axis=1)
    _, counts = np.unique(e[:, 0] << 32 | e[:, 1], return_counts=True)
    return int((counts == 1).sum())


# PsShell / PsShellsInfo (include/parsip_gpu.h), field for field
SHELL_DTYPE = np.dtype([("firstVertex", "<u4"), ("ctVertices", "<u4"), ("ctTriangles", "<u4"), ("ctEdges", "<u4"),
                        ("ctOpenEdges", "<u4"), ("ctNonManifoldEdges", "<u4"), ("ctFlippedEdges", "<u4"),
                        ("euler", "<i4"), ("area", "<f8"), ("volume", "<f8"),
                        ("bboxLo", "<f4", (3,)), ("bboxHi", "<f4", (3,))])
SHELLS_INFO_DTYPE = np.dtype([("ctShells", "<u4"), ("ctClosedShells", "<u4"), ("ctVertices", "<u4"),
                              ("ctTriangles", "<u4"), ("ctEdges", "<u4"), ("ctOpenEdges", "<u4"),
                              ("ctNonManifoldEdges", "<u4"), ("ctFlippedEdges", "<u4"), ("euler", "<i4"),
                              ("reserved", "<u4"), ("area", "<f8"), ("volume", "<f8"),
                              ("bboxLo", "<f4", (3,)), ("bboxHi", "<f4", (3,))])
assert SHELL_DTYPE.itemsize == 72 and SHELLS_INFO_DTYPE.itemsize == 80


@dataclass
class Shells:
    """What `shells` returns (and, from the device, `gpu.Polygonizer.weld_shells`)."""
    shells: np.ndarray        # (ctShells,) SHELL_DTYPE, ordered by firstVertex
    info: np.ndarray          # 0-d SHELLS_INFO_DTYPE: the whole mesh
    vertex_shell: np.ndarray  # (V,) u32: shell index of each vertex
    tri_shell: np.ndarray     # (T,) u32

    def tobytes(self) -> bytes:
        return b"".join(np.ascontiguousarray(a).tobytes()
                        for a in (self.shells, self.info, self.vertex_shell, self.tri_shell))


def shell_scales(pos, n_triangles: int):
    """The fixed-point exponents (eA, eV) of the shells' area and volume sums (parsip_gpu.h,
    "Reproducible measures"): M the largest |coordinate|, k the smallest integer with M < 2^k
    (0 for M = 0), L = ceil(log2(max(T, 2)))."""
    p = np.ascontiguousarray(pos, np.float32)
    big = float(np.abs(p).max()) if p.size else 0.0
    k = int(np.frexp(big)[1]) if big > 0.0 else 0   # big = m 2^k, 0.5 <= m < 1
    ell = (max(int(n_triangles), 2) - 1).bit_length()
    return 58 - 2 * k - ell, 58 - 3 * k - ell


def shell_terms(pos, tris):
    """Per triangle, A2 (twice its area) and V6 (six times its signed volume towards the
    origin) in float64 from the float32 positions, in the header's written-out order."""
    p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(tris).astype(np.int64).reshape(-1, 3)
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    bx, by, bz = b[:, 0], b[:, 1], b[:, 2]
    cx, cy, cz = c[:, 0], c[:, 1], c[:, 2]
    ux, uy, uz = bx - ax, by - ay, bz - az
    vx, vy, vz = cx - ax, cy - ay, cz - az
    nx, ny, nz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
    a2 = np.sqrt(nx * nx + ny * ny + nz * nz)
    v6 = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)
    return a2, v6


def shell_split(x, e: int):
    """x 2^e as (hi, lo) int64: hi = floor(y), lo = floor((y - hi) 2^30)."""
    y = np.ldexp(np.asarray(x, np.float64), e)
    hi = np.floor(y)
    lo = np.floor((y - hi) * float(1 << 30))
    return hi.astype(np.int64), lo.astype(np.int64)


def shell_join(hi, lo, e: int, div: float):
    """The value of two accumulators: (ldexp(hi, -e) + ldexp(lo, -e - 30)) / div."""
    return (np.ldexp(np.asarray(hi, np.int64).astype(np.float64), -e) +
            np.ldexp(np.asarray(lo, np.int64).astype(np.float64), -e - 30)) / div


def _float_order(a):
    """float32 -> u32 keys that order as the floats do, -0 below +0 (the device's min / max)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _float_unorder(k):
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def _components(n: int, a, b) -> np.ndarray:
    """Smallest vertex id of the connected component of each of n vertices under edges a-b."""
    lab = np.arange(n, dtype=np.int64)
    while len(a):
        new = lab.copy()
        la, lb = lab[a], lab[b]
        m = np.minimum(la, lb)
        np.minimum.at(new, la, m)   # hook the larger root under the smaller
        np.minimum.at(new, lb, m)
        while True:                 # flatten
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, lab):
            break
        lab = new
    return lab


def shells(pos, tris=None) -> Shells:
    """The shells (connected components) of an indexed mesh with their topology, area and
    volume: the host form of psgpu_weld_shells, same rule (parsip_gpu.h), same bytes.
    ``shells(mesh)`` takes a TriMesh or a gpu.WeldedMesh, ``shells(pos, tris)`` the arrays."""
    if tris is None:
        pos, tris = pos.pos, pos.tris
    p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    t = np.asarray(tris).astype(np.int64).reshape(-1, 3)
    V, T = len(p), len(t)
    if T and (t.min() < 0 or t.max() >= V):
        raise ValueError("a triangle names a vertex the mesh does not have")
    info = np.zeros((), SHELLS_INFO_DTYPE)
    if V == 0:
        return Shells(np.zeros(0, SHELL_DTYPE), info, np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    root = _components(V, np.concatenate([t[:, 0], t[:, 1]]), np.concatenate([t[:, 1], t[:, 2]]))
    first = np.flatnonzero(root == np.arange(V))
    S = len(first)
    index = np.zeros(V, np.int64)
    index[first] = np.arange(S)
    vs = index[root]
    ts = vs[t[:, 0]]
    out = np.zeros(S, SHELL_DTYPE)
    out["firstVertex"] = first
    out["ctVertices"] = np.bincount(vs, minlength=S)
    out["ctTriangles"] = np.bincount(ts, minlength=S)
    # edges: uses a -> b of every triangle, none for a == b
    ea = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    eb = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    use = ea != eb
    ea, eb = ea[use], eb[use]
    key, inv = np.unique(np.minimum(ea, eb) << 32 | np.maximum(ea, eb), return_inverse=True)
    inv = inv.reshape(-1)
    f = np.bincount(inv[ea < eb], minlength=len(key))
    b = np.bincount(inv[ea > eb], minlength=len(key))
    es = vs[key >> 32]
    out["ctEdges"] = np.bincount(es, minlength=S)
    out["ctOpenEdges"] = np.bincount(es[f + b == 1], minlength=S)
    out["ctFlippedEdges"] = np.bincount(es[(f + b == 2) & (f != b)], minlength=S)
    out["ctNonManifoldEdges"] = np.bincount(es[f + b >= 3], minlength=S)
    out["euler"] = (out["ctVertices"].astype(np.int64) - out["ctEdges"] + out["ctTriangles"]).astype(np.int32)
    # measures: exact integer sums of the split terms
    e_a, e_v = shell_scales(p, T)
    a2, v6 = shell_terms(p, t)
    acc = np.zeros((4, S), np.int64)
    for row, (x, e) in enumerate(((a2, e_a), (v6, e_v))):
        hi, lo = shell_split(x, e)
        np.add.at(acc[2 * row], ts, hi)
        np.add.at(acc[2 * row + 1], ts, lo)
    out["area"] = shell_join(acc[0], acc[1], e_a, 2.0)
    out["volume"] = shell_join(acc[2], acc[3], e_v, 6.0)
    keys = _float_order(p)
    lo_k = np.full((S, 3), 0xFFFFFFFF, np.uint32)
    hi_k = np.zeros((S, 3), np.uint32)
    np.minimum.at(lo_k, vs, keys)
    np.maximum.at(hi_k, vs, keys)
    out["bboxLo"], out["bboxHi"] = _float_unorder(lo_k), _float_unorder(hi_k)
    closed = ((out["ctOpenEdges"] == 0) & (out["ctFlippedEdges"] == 0) & (out["ctNonManifoldEdges"] == 0) &
              (out["ctTriangles"] > 0))
    info["ctShells"], info["ctClosedShells"] = S, int(closed.sum())
    for name in ("ctVertices", "ctTriangles", "ctEdges", "ctOpenEdges", "ctNonManifoldEdges", "ctFlippedEdges"):
        info[name] = out[name].astype(np.int64).sum()
    info["euler"] = int(info["ctVertices"]) - int(info["ctEdges"]) + int(info["ctTriangles"])
    tot = acc.sum(axis=1)
    info["area"] = shell_join(tot[0], tot[1], e_a, 2.0)
    info["volume"] = shell_join(tot[2], tot[3], e_v, 6.0)
    info["bboxLo"], info["bboxHi"] = _float_unorder(lo_k.min(axis=0)), _float_unorder(hi_k.max(axis=0))
    return Shells(out, info, vs.astype(np.uint32), ts.astype(np.uint32))


# PsShellFilter (include/parsip_gpu.h), field for field, and its flags
SHELL_FILTER_DTYPE = np.dtype([("flags", "<u4"), ("minVertices", "<u4"), ("minTriangles", "<u4"), ("reserved", "<u4"),
                               ("minArea", "<f8"), ("minAbsVolume", "<f8")])
assert SHELL_FILTER_DTYPE.itemsize == 32
FILTER_CLOSED_ONLY = 1
FILTER_DROP_CAVITIES = 2
DROPPED = 0xFFFFFFFF   # vertex_map / shell_map of what a filter drops


def shell_filter(criteria=None, **fields) -> np.ndarray:
    """A PsShellFilter as a 0-d SHELL_FILTER_DTYPE: ``criteria`` (None: all zero; a mapping or
    such an array) updated by ``fields``; ValueError on what psgpu_weld_filter refuses (an
    unknown field or flag bit, reserved != 0, a NaN, infinite or negative minArea / minAbsVolume)."""
    c = np.zeros((), SHELL_FILTER_DTYPE)
    if criteria is not None and not isinstance(criteria, dict):
        criteria = {k: criteria[k] for k in SHELL_FILTER_DTYPE.names}
    for k, v in dict(criteria or {}, **fields).items():
        if k not in SHELL_FILTER_DTYPE.names:
            raise ValueError(f"PsShellFilter has no field {k!r}")
        c[k] = v
    if int(c["flags"]) & ~(FILTER_CLOSED_ONLY | FILTER_DROP_CAVITIES) or c["reserved"] != 0:
        raise ValueError("unknown filter flags, or reserved != 0")
    for k in ("minArea", "minAbsVolume"):
        if not (np.isfinite(c[k]) and c[k] >= 0.0):
            raise ValueError(f"{k} must be finite and >= 0")
    return c


@dataclass
class FilteredMesh:
    """What `filter_shells` returns (and, from the device, `gpu.Polygonizer.weld_filter`)."""
    pos: np.ndarray         # (Vf, 3) f32: the kept vertices, in order
    nrm: np.ndarray
    col: np.ndarray
    tris: np.ndarray        # (Tf, 3) u32: the kept triangles, in order, filtered vertex ids
    vertex_map: np.ndarray  # (V,) u32: filtered id of every input vertex, DROPPED if it is dropped
    shell_map: np.ndarray   # (S,) u32: new index of every shell, DROPPED if it is dropped
    shells: np.ndarray      # (Sf,) SHELL_DTYPE: the kept records, firstVertex remapped

    def tobytes(self) -> bytes:
        return b"".join(np.ascontiguousarray(a).tobytes() for a in
                        (self.pos, self.nrm, self.col, self.tris, self.vertex_map, self.shell_map, self.shells))


def shells_kept(shells: np.ndarray, criteria=None, mask=None) -> np.ndarray:
    """psgpu_weld_filter's rule (parsip_gpu.h): which PsShell records a filter keeps, as bools;
    plain IEEE comparisons of the fields as stored."""
    c = shell_filter(criteria)
    sh = np.asarray(shells, SHELL_DTYPE)
    keep = np.ones(len(sh), bool)
    if mask is not None:
        m = np.asarray(mask)
        if m.shape != (len(sh),):
            raise ValueError(f"the mask has {m.size} entries, there are {len(sh)} shells")
        keep &= m != 0
    closed = ((sh["ctTriangles"] > 0) & (sh["ctOpenEdges"] == 0) & (sh["ctFlippedEdges"] == 0) &
              (sh["ctNonManifoldEdges"] == 0))
    keep &= (sh["ctVertices"] >= c["minVertices"]) & (sh["ctTriangles"] >= c["minTriangles"])
    keep &= (sh["area"] >= c["minArea"]) & (np.abs(sh["volume"]) >= c["minAbsVolume"])
    if int(c["flags"]) & FILTER_CLOSED_ONLY:
        keep &= closed
    if int(c["flags"]) & FILTER_DROP_CAVITIES:
        keep &= ~(closed & (sh["volume"] < 0.0))
    return keep


def _compact_map(keep: np.ndarray) -> np.ndarray:
    """Stable compaction: the new index of every kept element, DROPPED for the others."""
    out = np.full(len(keep), DROPPED, np.uint32)
    out[keep] = np.arange(int(keep.sum()), dtype=np.uint32)
    return out


def filter_shells(pos, nrm, col, tris, shells: Shells, criteria=None, mask=None) -> FilteredMesh:
    """The mesh without the shells a filter drops: the host form of psgpu_weld_filter, same rule
    (parsip_gpu.h), same bytes.  ``shells`` is the mesh's `Shells` (`shells(pos, tris)`, or a
    device download), ``criteria`` what `shell_filter` takes, ``mask`` one entry per shell.
    Kept vertices and triangles stay in order; the kept records keep the measures of the
    unfiltered mesh."""
    p = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(nrm, np.float32).reshape(-1, 3)
    c = np.ascontiguousarray(col, np.float32)
    c = c.reshape(-1, c.shape[-1] if c.ndim > 1 else 3)  # rgb, or the compat mode's rgba rows
    t = np.asarray(tris).astype(np.int64).reshape(-1, 3)
    if not (len(n) == len(c) == len(p) == len(shells.vertex_shell)) or len(t) != len(shells.tri_shell):
        raise ValueError("the shells are not those of this mesh")
    keep = shells_kept(shells.shells, criteria, mask)
    kv, kt = keep[shells.vertex_shell], keep[shells.tri_shell]
    vertex_map = _compact_map(kv)
    ftris = vertex_map[t[kt]].reshape(-1, 3)
    if (ftris == DROPPED).any():
        raise ValueError("a kept triangle names a dropped vertex")
    out = np.asarray(shells.shells, SHELL_DTYPE)[keep].copy()
    out["firstVertex"] = vertex_map[out["firstVertex"]]
    return FilteredMesh(p[kv], n[kv], c[kv], ftris, vertex_map, _compact_map(keep), out)


def _fmt(a) -> str:
    return " ".join(f"{float(x):.9g}" for x in a)


def write_off(mesh: TriMesh, path: str) -> None:
    """CMeshVV::save OFF (PS_MeshVV.cpp:1086-1108)."""
    with open(path, "w") as f:
        f.write("OFF\n")
        f.write(f"{mesh.n_vertices} {mesh.n_triangles} {mesh.n_triangles * 3}\n")
        for p in mesh.pos:
            f.write(_fmt(p) + " \n")
        for t in mesh.tris:
            f.write(f"3 {t[0]} {t[1]} {t[2]} \n")


def write_ply(mesh: TriMesh, path: str) -> None:
    """CMeshVV::save ASCII PLY (PS_MeshVV.cpp:1109-1143)."""
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\n")
        f.write(f"element vertex {mesh.n_vertices}\n")
        f.write("property float32 x\nproperty float32 y\nproperty float32 z\n")
        f.write(f"element face {mesh.n_triangles}\n")
        f.write("property list uint8 int32 vertex_indices\nend_header\n")
        for p in mesh.pos:
            f.write(_fmt(p) + " \n")
        for t in mesh.tris:
            f.write(f"3 {t[0]} {t[1]} {t[2]} \n")


def write_obj(mesh: TriMesh, path: str) -> None:
    """Wavefront OBJ with per-vertex normals (1-based ids)."""
    with open(path, "w") as f:
        f.write(f"# parsip_amd mesh: {mesh.n_vertices} vertices, {mesh.n_triangles} triangles\n")
        for p in mesh.pos:
            f.write("v " + _fmt(p) + "\n")
        if mesh.nrm is not None:
            for n in mesh.nrm:
                f.write("vn " + _fmt(n) + "\n")
            for t in mesh.tris + 1:
                f.write(f"f {t[0]}//{t[0]} {t[1]}//{t[1]} {t[2]}//{t[2]}\n")
        else:
            for t in mesh.tris + 1:
                f.write(f"f {t[0]} {t[1]} {t[2]}\n")


def read_off(path: str) -> TriMesh:
    with open(path) as f:
        toks = f.read().split()
    assert toks[0] == "OFF"
    nv, nt = int(toks[1]), int(toks[2])
    vals = toks[4:]
    pos = np.array(vals[:nv * 3], np.float32).reshape(-1, 3)
    faces = np.array(vals[nv * 3:nv * 3 + nt * 4], np.int64).reshape(-1, 4)
    return TriMesh(pos, faces[:, 1:])
