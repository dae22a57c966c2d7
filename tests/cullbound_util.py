"""Inputs and the CPU-side model shared by the box-bound tests (test_cullbound.py on the CPU,
test_gpu_cullbound.py on the device) and tools/cull_pairs.py: tests/cpp/cullbound_check.cpp, which
compiles the culling predicate and the primitive field interval of psgpu_model.h, the sphere form
and the box form of each, as plain C++ and runs them on the device image of a model
(gpu.model_image: host only)."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

from parsip_amd import gpu, soa, synth
from parsip_amd.soa import NodeType

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cullbound_counts.json")
F = np.float32
KINDS = (NodeType.POINT, NodeType.LINE, NodeType.CYLINDER, NodeType.CUBE)
COLUMNS = ("all", "cube", "point", "cylinder", "line")

_EXE = {}


def check_exe(sanitize: bool = False) -> str:
    """tests/cpp/cullbound_check.cpp compiled with g++ (no HIP, no contraction), once per session;
    sanitize: with AddressSanitizer and UBSan (a plain program of its own: nothing is preloaded)."""
    key = "san" if sanitize else "exe"
    if key not in _EXE:
        gpp = shutil.which("g++")
        assert gpp is not None, "g++ is needed to compile tests/cpp/cullbound_check.cpp"
        d = tempfile.mkdtemp(prefix="cullbound_")
        exe = os.path.join(d, "cullbound_check")
        extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
        subprocess.run([gpp, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", *extra, "-I",
                        os.path.join(ROOT, "parsip_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "cullbound_check.cpp"), "-o", exe], check=True)
        _EXE[key] = exe
    return _EXE[key]


class Check:
    """What cullbound_check says of a model: of a list of boxes, and (cs given) of its lattice."""

    def __init__(self, model, tag: str, boxes=None, cs: float | None = None, seed: int = 0, sanitize: bool = False):
        boxes = np.zeros((0, 6), F) if boxes is None else np.ascontiguousarray(boxes, F).reshape(-1, 6)
        if cs is None:
            dims, org, cs = (0, 0, 0), np.zeros((0, 3), F), 1.0
        else:
            dims = tuple(int(x) for x in soa.mpu_dims(cs, *model.bbox))
            org = soa.mpu_origins(cs, *model.bbox).astype(F)
        self.dims = dims
        exe = check_exe(sanitize)
        d = os.path.dirname(exe)
        src, out = os.path.join(d, tag + ".in"), os.path.join(d, tag + ".out")
        with open(src, "wb") as f:
            f.write(np.array([len(boxes), len(org), *dims, seed], np.uint32).tobytes())
            f.write(np.asarray(model.bbox[0], F).tobytes() + F(cs).tobytes())
            f.write(gpu.model_image(model))
            f.write(boxes.tobytes() + np.ascontiguousarray(org, F).tobytes())
        r = subprocess.run([exe, src, out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stderr)
        self.stderr = r.stderr
        raw = open(out, "rb").read()
        w = np.frombuffer(raw[:8 * 30], np.uint64)
        (self.pairs_tested, self.culled_sphere, self.culled_box, self.unsound_culls, self.lost_culls,
         self.intervals_tested, self.unsound_intervals, self.wider_intervals) = (int(x) for x in w[:8])
        self.live = w[8:28].reshape(2, 2, 5).astype(np.int64)  # [MPU boxes, bricks][sphere, box][COLUMNS]
        self.dead_bricks = tuple(int(x) for x in w[28:30])
        v = np.frombuffer(raw[8 * 30:], np.uint8).reshape(-1, 4).astype(bool)
        self.zero_sphere, self.zero_box, self.proven_sphere, self.proven_box = (v[:, k] for k in range(4))

    def counts(self) -> dict:
        """The live-pair table (tools/cull_pairs.py, tests/golden/cullbound_counts.json)."""
        out = {}
        for w, where in enumerate(("mpu_boxes", "brick_boxes")):
            for v, form in enumerate(("sphere", "box")):
                out[f"{where}_{form}"] = {c: int(self.live[w, v, k]) for k, c in enumerate(COLUMNS)}
        out["dead_bricks_sphere"], out["dead_bricks_box"] = self.dead_bricks
        out["proven_empty_sphere"] = int(np.count_nonzero(self.proven_sphere))
        out["proven_empty_box"] = int(np.count_nonzero(self.proven_box))
        return out


def coarse(name: str, cells: int):
    model, cs, n = synth.make_config(name)
    return model, float(F(cs * n / cells))


def prim_soup(seed: int, scale: float = 1.0, offset=(0.0, 0.0, 0.0)) -> soa.Model:
    """128 primitives of the four cullable types with random finite parameters under no op (the
    sum of the primitives): positions within `scale` of `offset`, sizes up to `scale`."""
    rng = np.random.default_rng(seed)
    m = soa.Model.empty(f"soup{seed}")
    P = m.prims
    for i in range(128):
        t = KINDS[i % 4] if i < 96 else int(rng.choice(KINDS))
        c = (np.asarray(offset) + rng.uniform(-scale, scale, 3)).astype(F)
        synth.set_prim(m, i, t, c)
        if t == NodeType.LINE:
            e = c + (rng.uniform(-1, 1, 3) * scale).astype(F)
            if i % 8 == 1:  # parallel to an axis
                e = c.copy()
                e[int(rng.integers(0, 3))] += F(scale * rng.uniform(0.2, 1.0))
            P["dirX"][0, i], P["dirY"][0, i], P["dirZ"][0, i] = e
        elif t == NodeType.CYLINDER:
            d = rng.normal(size=3)
            if i % 8 == 2:
                d = np.eye(3)[int(rng.integers(0, 3))] * rng.choice((-1.0, 1.0))
            d = (d / np.linalg.norm(d)).astype(F)
            P["dirX"][0, i], P["dirY"][0, i], P["dirZ"][0, i] = d
            P["resX"][0, i], P["resY"][0, i] = rng.uniform(0.0, 0.6) * scale, rng.uniform(0.01, 1.5) * scale
        elif t == NodeType.CUBE:
            P["resX"][0, i] = rng.uniform(0.0, 0.7) * scale
    P["ctPrims"][0] = 128
    synth.prepare_boxes(m)
    m.prims["bboxLo"][0] = tuple(np.asarray(offset, F) - F(3 * scale))
    m.prims["bboxHi"][0] = tuple(np.asarray(offset, F) + F(3 * scale))
    return m


def prim_geometry(model):
    """pos, dir, res (n, 3) and type (n) of a model's primitives."""
    P, n = model.prims, model.ct_prims
    pos = np.stack([P[f"pos{c}"][0, :n] for c in "XYZ"], 1).astype(F)
    dr = np.stack([P[f"dir{c}"][0, :n] for c in "XYZ"], 1).astype(F)
    res = np.stack([P[f"res{c}"][0, :n] for c in "XYZ"], 1).astype(F)
    return pos, dr, res, np.asarray(P["skeletType"][0, :n]).astype(int)


def adversarial_boxes(model, seed: int, scale: float = 1.0) -> np.ndarray:
    """Boxes {x0, y0, z0, x1, y1, z1} round a model's primitives: octant, MPU and brick sizes at
    random places and at the distance where the field ends; flat and degenerate boxes; boxes of
    1e6 times the scale; boxes that contain a primitive; boxes centred exactly on a Point; boxes
    a Cylinder's axis or a Line crosses; boxes whose faces coincide with a Cube's."""
    rng = np.random.default_rng(seed)
    pos, dr, res, typ = prim_geometry(model)
    centre = pos.mean(0)
    cs = 0.0625 * scale
    out = []

    def box(c, h):
        c, h = np.asarray(c, np.float64), np.abs(np.asarray(h, np.float64)) * np.ones(3)
        out.append(np.concatenate([(c - h).astype(F), (c + h).astype(F)]))

    sizes = (1.5 * cs, 3.5 * cs + 0.0005, 7 * cs, 14 * cs)  # octant, MPU, brick halves
    for _ in range(160):
        box(centre + rng.uniform(-3, 3, 3) * scale, rng.choice(sizes))
    for i in range(len(pos)):
        p, s = pos[i].astype(np.float64), float(res[i, 0])
        for h in sizes[:3]:
            # face-on, edge-on and corner-on, at the distance where dist2 crosses 1 (the unit is
            # the field's support, not `scale`) and a little either side of it
            for dirn in ((1, 0, 0), (0, -1, 0), (1, 1, 0), (0, 1, -1), (1, -1, 1)):
                dirn = np.asarray(dirn, np.float64)
                reach = 1.0 + (s if typ[i] in (NodeType.CUBE, NodeType.CYLINDER) else 0.0)
                for eps in (-0.05, 0.0, 0.012, 0.05):
                    box(p + dirn * (reach + h + eps), h)
        box(p, sizes[1])                                   # contains the primitive's anchor
        box(p, (s + 2.0) * max(scale, 1.0))                # contains all of it but a Line
        box(p, (sizes[0], 0.0, sizes[2]))                  # flat, centred on it
        box(p + rng.uniform(-1.5, 1.5, 3), (0.0, 0.0, 0.0))    # a single point
        box(p + rng.uniform(-1.5, 1.5, 3), (sizes[2], 0.0, 0.0))   # a segment
        box(p + rng.uniform(-2, 2, 3) * 1e6 * scale, 1e6 * scale * rng.uniform(0.1, 2.0, 3))
        box(p, 1e6 * scale)
        if typ[i] == NodeType.CUBE:
            lo, hi = p - s, p + s
            out.append(np.concatenate([lo, hi]).astype(F))                         # the cube itself
            out.append(np.concatenate([[hi[0], lo[1], lo[2]], [hi[0] + 2 * sizes[1], hi[1], hi[2]]]).astype(F))
            out.append(np.concatenate([[hi[0] + 1.01, lo[1], lo[2]], [hi[0] + 1.01 + sizes[0], hi[1], hi[2]]]).astype(F))
        if typ[i] in (NodeType.CYLINDER, NodeType.LINE):
            u = dr[i].astype(np.float64) if typ[i] == NodeType.CYLINDER else dr[i].astype(np.float64) - p
            for t in (-0.7, 0.3, 1.9):
                box(p + t * u, rng.choice(sizes))              # the axis crosses the box
                off = np.cross(u, rng.normal(size=3))
                off /= max(np.linalg.norm(off), 1e-9)
                box(p + t * u + off * (1.0 + s + sizes[1] * 1.2), sizes[1])  # beside it, near the field's end
    return np.asarray(out, F)


def only_tree(kind: int, cs: float, seed: int):
    """Eight primitives of one type under a balanced tree, placed so that they touch MPU faces of
    the lattice of cell size cs over [-2, 2]^3: a Cube's faces, a Cylinder's caps and a Line lie
    on MPU faces (Lines parallel to an axis)."""
    rng = np.random.default_rng(seed)
    m = soa.Model.empty(f"only{kind}")
    P = m.prims
    side = 7.0 * cs
    for i in range(8):
        face = -2.0 + side * rng.integers(1, int(4.0 / side), 3)  # MPU faces of the lattice
        c = face.astype(F)
        synth.set_prim(m, i, kind, c)
        if kind == NodeType.CUBE:
            s = F(side * (0.5 if i % 2 else 1.0))
            P["resX"][0, i] = s
            c = (face + (s if i % 4 < 2 else 0.0)).astype(F)
            P["posX"][0, i], P["posY"][0, i], P["posZ"][0, i] = c
        elif kind == NodeType.CYLINDER:
            d = np.eye(3)[i % 3].astype(F)
            P["dirX"][0, i], P["dirY"][0, i], P["dirZ"][0, i] = d
            P["resX"][0, i], P["resY"][0, i] = F(0.5 * side if i % 2 else 0.2), F(side)
        elif kind == NodeType.LINE:
            e = c.copy()
            e[i % 3] += F(side)
            P["dirX"][0, i], P["dirY"][0, i], P["dirZ"][0, i] = e
    P["ctPrims"][0] = 8
    synth.build_balanced_ops(m, 8)
    synth.prepare_boxes(m)
    m.prims["bboxLo"][0] = (-2.0, -2.0, -2.0)
    m.prims["bboxHi"][0] = (2.0, 2.0, 2.0)
    return m
