"""Inputs and CPU-side references shared by the op-inside mask tests (test_op_inside.py on the
CPU, test_gpu_op_inside.py on the device): trees with ops deeper than 3 (C1 and C2 have none),
the masks of tests/cpp/op_inside_check.cpp, and the points the walks evaluate under an MPU."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

from parsip_amd import soa, synth
from parsip_amd.soa import NodeType

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def chain_model(seed: int, n_prims: int, offset, spread: float, half: float) -> soa.Model:
    """An unbalanced tree: op k's left child is op k + 1, its right child primitive k (op k is at
    depth k, so a 12-primitive chain is 11 deep), primitives placed by a seeded walk of short
    steps so that the deep ops' boxes are tight (a few MPUs across), the whole scene moved by
    `offset` (large coordinates: the margin's magnitude term and the fp32 lattice are exercised)."""
    rng = np.random.default_rng(seed)
    m = soa.Model.empty(f"chain{seed}")
    c = np.zeros(3)
    types = (NodeType.POINT, NodeType.CUBE, NodeType.POINT, NodeType.LINE)
    for i in range(n_prims):
        c = np.clip(c + rng.uniform(-spread, spread, 3), -0.5 * half, 0.5 * half)
        synth.set_prim(m, i, types[i % 4], (c + np.asarray(offset)).astype(F))
        if types[i % 4] == NodeType.LINE:
            e = (c + np.asarray(offset) + rng.uniform(-0.3, 0.3, 3)).astype(F)
            m.prims["dirX"][0, i], m.prims["dirY"][0, i], m.prims["dirZ"][0, i] = e
        elif types[i % 4] == NodeType.CUBE:
            m.prims["resX"][0, i] = F(0.2)
    m.prims["ctPrims"][0] = n_prims
    O = m.ops
    for k in range(n_prims - 1):
        last = k == n_prims - 2
        O["opType"][0, k] = (NodeType.UNION, NodeType.BLEND, NodeType.BLEND, NodeType.DIF)[k % 4] if k else NodeType.UNION
        O["opLeftChild"][0, k] = n_prims - 1 if last else k + 1
        O["opRightChild"][0, k] = k
        O["opChildKind"][0, k] = 0 if last else 2
    O["ctOps"][0] = n_prims - 1
    synth.prepare_boxes(m)
    m.prims["bboxLo"][0] = (np.asarray(offset) - half).astype(F)
    m.prims["bboxHi"][0] = (np.asarray(offset) + half).astype(F)
    return m


def _coarse(name: str, cells: int):
    model, cs, n = synth.make_config(name)
    return model, float(F(cs * n / cells))


def _off_round(name: str, cs: float):
    return synth.make_config(name)[0], cs


# name -> () -> (model, cellsize): C3 and C5 at a 64^3 lattice and at one off-round cell size, and
# two seeded chains with tight boxes far from the origin
CASES = {
    "C3_64": lambda: _coarse("C3", 64),
    "C5_64": lambda: _coarse("C5", 64),
    "C3_0.0713": lambda: _off_round("C3", 0.0713),
    "C5_0.0911": lambda: _off_round("C5", 0.0911),
    "chain7": lambda: (chain_model(7, 12, (1000.0, -500.0, 250.0), 0.35, 2.0), 0.0617),
    "chain11": lambda: (chain_model(11, 14, (-4096.0, 33.0, 8191.0), 0.5, 2.5), 0.0831),
}

_MODELS = {}


def make_case(name: str):
    if name not in _MODELS:
        _MODELS[name] = CASES[name]()
    return _MODELS[name]


def op_boxes(model):
    n = model.ct_ops
    lo = np.stack([model.ops[f"vBoxLo{c}"][0, :n] for c in "XYZ"], 1).astype(F)
    hi = np.stack([model.ops[f"vBoxHi{c}"][0, :n] for c in "XYZ"], 1).astype(F)
    return lo, hi


def op_depths(model) -> np.ndarray:
    d = np.zeros(model.ct_ops, np.int64)

    def rec(op, depth):
        d[op] = depth
        kind = int(model.ops["opChildKind"][0, op])
        if kind & 2:
            rec(int(model.ops["opLeftChild"][0, op]), depth + 1)
        if kind & 1:
            rec(int(model.ops["opRightChild"][0, op]), depth + 1)

    if model.ct_ops:
        rec(0, 0)
    return d


_EXE = {}


def check_exe() -> str:
    """tests/cpp/op_inside_check.cpp compiled with g++ (no HIP, no contraction), once per session."""
    if "exe" not in _EXE:
        gpp = shutil.which("g++")
        assert gpp is not None, "g++ is needed to compile tests/cpp/op_inside_check.cpp"
        d = tempfile.mkdtemp(prefix="op_inside_")
        exe = os.path.join(d, "op_inside_check")
        subprocess.run([gpp, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-I",
                        os.path.join(ROOT, "parsip_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "op_inside_check.cpp"),
                        "-o", exe], check=True)
        _EXE["exe"] = exe
    return _EXE["exe"]


_MASKS = {}


def cpu_masks(name: str) -> np.ndarray:
    """(MPUs, 2) uint64: the predicate of psgpu_model.h for every MPU of the lattice and every op."""
    if name not in _MASKS:
        model, cs = make_case(name)
        lo, hi = op_boxes(model)
        org = soa.mpu_origins(cs, *model.bbox)
        d = os.path.dirname(check_exe())
        src, out = os.path.join(d, name + ".in"), os.path.join(d, name + ".out")
        with open(src, "wb") as f:
            f.write(np.array([len(lo), len(org)], np.uint32).tobytes() + F(cs).tobytes() + np.uint32(0).tobytes())
            f.write(np.concatenate([lo, hi], 1).astype(F).tobytes() + org.astype(F).tobytes())
        r = subprocess.run([check_exe(), src, out], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        _MASKS[name] = np.fromfile(out, np.uint64).reshape(-1, 2)
    return _MASKS[name]


def mask_bits(masks: np.ndarray, n_ops: int) -> np.ndarray:
    """(MPUs, n_ops) bool from (MPUs, 2) uint64 words."""
    k = np.arange(n_ops)
    words = masks[:, k >> 6]
    return ((words >> (k & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def ref_in(pts: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """The reference's per-point op-box test (PS_Polygonizer.cpp:1228-1252), fp32 compares:
    pts (n, 3), boxes (k, 3) -> (n, k) bool, true when the point is inside along any axis."""
    p = pts.astype(F)[:, None, :]
    return ((p >= lo[None]) & (hi[None] >= p)).any(2)


def corner_coords(org: np.ndarray, cs: float) -> np.ndarray:
    """(MPUs, 3, 8): the S2 corner coordinates o + (float)i * cs per axis."""
    step = (np.arange(8, dtype=F) * F(cs)).astype(F)
    return (org[:, :, None] + step[None, None, :]).astype(F)


def vertex_points(pos: np.ndarray, org: np.ndarray, cs: float) -> np.ndarray:
    """The points k_vertex and k_finish walk for the oracle vertices `pos` of the MPU at `org`:
    per vertex its lattice edge's four samples e1 + (e2 - e1) * (l / 3) (PS_Polygonizer.cpp:722-755),
    the root and the three normal points root + 0.001 e_a (:780-781), (points, 3).  The edge is
    found from the position: two coordinates equal S2 corner coordinates bit for bit, the third
    lies between two neighbouring ones (on a corner itself: that axis counts as the edge's).
    A root the reference's linear extrapolation put off its segment and outside the MPU's extent
    (scale outside [0, 1]) is not one of the points: k_finish walks such waves with the mask of
    their own box, whose op-inside words are 0; its edge is then unknown, so the samples of all
    7 edges along that axis stand in for it."""
    cs = F(cs)
    third = F(1.0) / F(3.0)
    cc = corner_coords(org[None], cs)[0]  # (3, 8)
    out = []
    for p in pos.astype(F):
        on = [np.flatnonzero(cc[a] == p[a]) for a in range(3)]
        free = [a for a in range(3) if len(on[a]) == 0]
        assert len(free) <= 1, (p, org)
        ax = free[0] if free else 0
        inside = cc[ax][0] <= p[ax] <= cc[ax][7]
        s = [int(on[a][0]) if len(on[a]) else 0 for a in range(3)]
        first = int(min(max(np.searchsorted(cc[ax], p[ax], side="right") - 1, 0), 6))
        for s[ax] in ([first] if inside else range(7)):
            e = np.array([cc[a][s[a]] for a in range(3)], F)
            d = np.zeros(3, F)
            d[ax] = F(F(e[ax] + cs) - e[ax])
            out += [e + d * F(F(l) * third) for l in range(4)]
        if inside:
            out.append(p)
            for a in range(3):
                q = p.copy()
                q[a] = F(p[a] + F(0.001))
                out.append(q)
    return np.asarray(out, F).reshape(-1, 3)
