"""Inputs and the CPU-side model shared by the sieve tests (test_sieve.py on the CPU,
test_gpu_sieve.py on the device): tests/cpp/sieve_check.cpp, which compiles k_sieve's decision
(brick_box, cull_box, cull_one and the root-zero set of psgpu_model.h) as plain C++, run on the
device image of a model (gpu.model_image: host only)."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

from parsip_amd import gpu, soa, synth
from parsip_amd.soa import NodeType

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

TYPES = [NodeType.POINT, NodeType.LINE, NodeType.CYLINDER, NodeType.CUBE, NodeType.DISC, NodeType.RING,
         NodeType.TRIANGLE]
OPS = [NodeType.BLEND, NodeType.UNION, NodeType.INTERSECT, NodeType.DIF, NodeType.SMOOTHDIF, NodeType.RICCIBLEND,
       NodeType.GRADIENTBLEND, NodeType.WARPTWIST, NodeType.WARPTAPER, NodeType.WARPBEND, NodeType.WARPSHEAR]
CULLABLE = [NodeType.POINT, NodeType.LINE, NodeType.CYLINDER, NodeType.CUBE, NodeType.TRIANGLE]
ZERO_CLOSED = [NodeType.BLEND, NodeType.UNION, NodeType.INTERSECT, NodeType.DIF, NodeType.SMOOTHDIF,
               NodeType.WARPTWIST, NodeType.WARPTAPER, NodeType.WARPBEND, NodeType.WARPSHEAR]


def fuzz_tree(seed: int):
    """The fuzz generator's seeded trees (test_gpu_fuzz.py): every primitive and op type, warps,
    matrices; every third seed from the cullable primitives and the +0-closed ops only (without
    matrices), so that trees with a root-zero set are among them."""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(2, 25))
    if seed % 3 == 2:
        return synth.random_model(1000 + seed, n_prims=n, types=CULLABLE, op_types=ZERO_CLOSED, matrices=False)
    return synth.random_model(1000 + seed, n_prims=n, types=TYPES, op_types=OPS, matrices=bool(rng.integers(0, 2)))


def disc_tree():
    """Six points and one Disc (never culled) under Blends."""
    m = synth.random_model(77, n_prims=7, types=[NodeType.POINT])
    synth.set_prim(m, 3, NodeType.DISC, (0.3, -0.2, 0.1))
    P = m.prims
    P["dirX"][0, 3], P["dirY"][0, 3], P["dirZ"][0, 3] = 0.0, 0.0, 1.0
    P["resX"][0, 3], P["resY"][0, 3] = F(0.4), F(0.4) * F(0.4)
    synth.prepare_boxes(m)
    return m


def ricci_tree():
    """Cullable primitives only, under a Ricci root (not +0-closed)."""
    m = synth.random_model(78, n_prims=6, types=[NodeType.POINT, NodeType.CUBE])
    m.ops["opType"][0, 0] = int(NodeType.RICCIBLEND)
    m.ops["resY"][0, 0] = F(1.5)
    synth.prepare_boxes(m)
    return m


def far_tree():
    """C2's tree moved far outside its lattice along z (across its lines, which are unbounded,
    and its cylinders' axes): no primitive reaches any brick."""
    m = synth.make_config("C2")[0].copy()
    m.prims["posZ"][0, :8] += F(1000.0)
    m.prims["dirZ"][0, 1:8:4] += F(1000.0)  # a line's second point
    synth.prepare_boxes(m)
    m.prims["bboxLo"][0] = (-4.0, -4.0, -4.0)
    m.prims["bboxHi"][0] = (4.0, 4.0, 4.0)
    return m


_EXE = {}


def check_exe() -> str:
    """tests/cpp/sieve_check.cpp compiled with g++ (no HIP, no contraction), once per session."""
    if "exe" not in _EXE:
        gpp = shutil.which("g++")
        assert gpp is not None, "g++ is needed to compile tests/cpp/sieve_check.cpp"
        d = tempfile.mkdtemp(prefix="sieve_")
        exe = os.path.join(d, "sieve_check")
        subprocess.run([gpp, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-I",
                        os.path.join(ROOT, "parsip_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "sieve_check.cpp"),
                        "-o", exe], check=True)
        _EXE["exe"] = exe
    return _EXE["exe"]


class Sieve:
    """What sieve_check says of a model at a cell size."""

    def __init__(self, model, cs: float, tag: str):
        self.dims = tuple(int(x) for x in soa.mpu_dims(cs, *model.bbox))
        self.nb = tuple((d + 1) // 2 for d in self.dims)
        d = os.path.dirname(check_exe())
        src, out = os.path.join(d, tag + ".in"), os.path.join(d, tag + ".out")
        with open(src, "wb") as f:
            f.write(np.asarray(model.bbox[0], F).tobytes() + F(cs).tobytes())
            f.write(np.array(list(self.dims) + [0], np.uint32).tobytes())
            f.write(gpu.model_image(model))
        r = subprocess.run([check_exe(), src, out], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.returncode, r.stderr)
        raw = open(out, "rb").read()
        self.valid, self.agree = (int(x) for x in np.frombuffer(raw[:8], np.uint32))
        self.root_zero = np.frombuffer(raw[8:24], np.uint64)
        self.dead = np.frombuffer(raw[24:], np.uint8).reshape(self.nb).astype(bool)

    def mpu_dead(self) -> np.ndarray:
        """Per MPU of the lattice (x-major, as the MPU ids): its brick is dead."""
        i, j, k = np.meshgrid(*(np.arange(d) for d in self.dims), indexing="ij")
        return self.dead[i // 2, j // 2, k // 2].reshape(-1)

    def live_set(self, begin: int = 0, end: int | None = None) -> set:
        """The bricks k_sieve lists for the MPU range [begin, end): not dead, and with an MPU of
        the range."""
        n = int(np.prod(self.dims))
        end = n if end is None else end
        inr = np.zeros(n, bool)
        inr[begin:end] = True
        i, j, k = np.meshgrid(*(np.arange(d) for d in self.dims), indexing="ij")
        has = np.zeros(self.nb, bool)
        np.logical_or.at(has, (i // 2, j // 2, k // 2), inr.reshape(self.dims))
        return {tuple(int(x) for x in b) for b in np.argwhere(has & ~self.dead)}
