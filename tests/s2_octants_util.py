"""Inputs and the CPU-side model shared by the S2 octant tests (test_s2_octants.py on the CPU,
test_gpu_s2_octants.py on the device) and tools/s2_octants.py: tests/cpp/s2_octants_check.cpp, which
compiles the S2 octant plan and the host model of S1's per-octant field verdicts (psgpu_model.h)
as plain C++ and runs them on the device image of a model (gpu.model_image: host only)."""
import os
import shutil
import subprocess
import tempfile

import numpy as np

import aniso_util
import cullbound_util as U
from parsip_amd import gpu, soa, synth
from parsip_amd.soa import NodeType
from sieve_util import fuzz_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "s2_octants_counts.json")
F = np.float32
ONLY = {"cubes": NodeType.CUBE, "cylinders": NodeType.CYLINDER, "lines": NodeType.LINE}
N_FUZZ = 40


def _c3_538():
    model = aniso_util.boxed(synth.make_config("C3")[0],
                             *aniso_util.box_for((5, 3, 8), aniso_util.FIRST, aniso_util.CS))
    return model, aniso_util.CS


# name -> () -> (model, cell size): C2, C3 at 64^3 cells, C3's tree in a 5x3x8 lattice, trees of
# one primitive type whose primitives touch MPU faces, the fuzz trees at 32^3 cells
CASES = {"C2": lambda: synth.make_config("C2")[:2], "C3_64": lambda: U.coarse("C3", 64), "C3_5x3x8": _c3_538}
CASES.update({f"only_{k}": (lambda t=t, i=i: (U.only_tree(t, 4.0 / 64, 40 + i), 4.0 / 64))
              for i, (k, t) in enumerate(ONLY.items())})
CASES.update({f"fuzz{s}": (lambda s=s: (fuzz_tree(s), 4.0 / 32)) for s in range(N_FUZZ)})

_MODELS, _EXE = {}, {}


def make_case(name):
    if name not in _MODELS:
        _MODELS[name] = CASES[name]()
    return _MODELS[name]


def tree_splits(model) -> bool:
    """The tree split applies to this tree (Gen::splittable, psgpu_jit.cpp): a binary root op
    (Union .. Ricci) over two ops, and no op of an unknown type anywhere."""
    O = model.ops
    n = int(O["ctOps"][0])
    if n == 0:
        return False
    types = [int(t) for t in O["opType"][0, :n]]
    known = all(14 <= t <= 19 or 22 <= t <= 25 for t in types)
    return known and int(O["opChildKind"][0, 0]) == 3 and 14 <= types[0] <= 19


def check_exe(sanitize: bool = False) -> str:
    """tests/cpp/s2_octants_check.cpp compiled with g++ (no HIP, no contraction), once per session;
    sanitize: with AddressSanitizer and UBSan (a plain program of its own: nothing is preloaded)."""
    key = "san" if sanitize else "exe"
    if key not in _EXE:
        gpp = shutil.which("g++")
        assert gpp is not None, "g++ is needed to compile tests/cpp/s2_octants_check.cpp"
        d = tempfile.mkdtemp(prefix="s2_octants_")
        exe = os.path.join(d, "s2_octants_check")
        extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
        subprocess.run([gpp, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", *extra, "-I",
                        os.path.join(ROOT, "parsip_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "s2_octants_check.cpp"), "-o", exe], check=True)
        _EXE[key] = exe
    return _EXE[key]


def plan_check(sanitize: bool = False):
    """The program's own check of the plan and the bit assembly: (exit code, stderr)."""
    r = subprocess.run([check_exe(sanitize), "plan"], capture_output=True, text=True, timeout=300)
    return r.returncode, r.stderr


class Verdicts:
    """The host model's per-octant verdicts of a model's lattice, given the MPUs that passed S1
    (the oracle's stats[:, 0]): queued, outside, inside (bit c = xh | yh << 1 | zh << 2), passes."""

    def __init__(self, model, cs: float, passed, tag: str, bound: bool = True, sanitize: bool = False):
        self.model, self.cs = model, float(F(cs))
        self.dims = tuple(int(x) for x in soa.mpu_dims(cs, *model.bbox))
        self.org = np.ascontiguousarray(soa.mpu_origins(cs, *model.bbox), F)
        passed = np.ascontiguousarray(np.asarray(passed) != 0, np.uint8)
        assert len(passed) == len(self.org) == int(np.prod(self.dims))
        exe = check_exe(sanitize)
        d = os.path.dirname(exe)
        src, out = os.path.join(d, tag + ".in"), os.path.join(d, tag + ".out")
        with open(src, "wb") as f:
            f.write(np.array([len(self.org), *self.dims, 1 if bound else 0], np.uint32).tobytes())
            f.write(np.asarray(model.bbox[0], F).tobytes() + F(cs).tobytes())
            f.write(gpu.model_image(model))
            f.write(self.org.tobytes() + passed.tobytes())
        r = subprocess.run([exe, src, out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stderr)
        v = np.frombuffer(open(out, "rb").read(), np.uint8).reshape(-1, 4)
        self.queued = v[:, 0].astype(bool)
        self.outside, self.inside, self.passes = v[:, 1].astype(int), v[:, 2].astype(int), v[:, 3].astype(int)

    def entry_words(self) -> np.ndarray:
        """Per MPU the 16 verdict bits its queue entry carries (outside | inside << 8), 0 if not queued."""
        return np.where(self.queued, self.outside | (self.inside << 8), 0).astype(np.uint16)

    def undecided(self) -> np.ndarray:
        """Per queued MPU, the count of its octants S1 left undecided (0..8)."""
        known = (self.outside | self.inside)[self.queued]
        return 8 - np.array([bin(int(k)).count("1") for k in known], int)

    def histogram(self) -> list:
        return [int(x) for x in np.bincount(self.undecided(), minlength=9)]

    def counts(self) -> dict:
        """The row of the model table (tools/s2_octants.py, tests/golden/s2_octants_counts.json)."""
        u = self.undecided()
        n = len(u)
        return {"queued": n, "undecided_histogram": self.histogram(),
                "mean_undecided": round(float(u.mean()), 4) if n else 0.0,
                "queued_le4_undecided": int(np.count_nonzero(u <= 4)),
                "passes": int(self.passes.sum()), "passes_all_octants": 2 * n,
                "points_walked": int(256 * self.passes.sum()), "points_all": 512 * n,
                "points_decided": int(64 * (8 - u).sum())}

    def decided_points(self):
        """The lattice points of every decided octant of every queued MPU, built with the
        device's fp32 expressions (o + (float)k * cs), in the reference's SIMD groups (4
        consecutive z at one (x, y)): x, y, z and whether the octant was proven inside."""
        cs = F(self.cs)
        k4 = np.arange(4)
        xs, ys, zs, ins = [], [], [], []
        for m in np.flatnonzero(self.queued):
            o = self.org[m]
            for c in range(8):
                side = (self.inside[m] >> c) & 1
                if not (((self.outside[m] >> c) & 1) or side):
                    continue
                kx, ky, kz = 4 * (c & 1) + k4, 4 * ((c >> 1) & 1) + k4, 4 * (c >> 2) + k4
                px = (o[0] + kx.astype(F) * cs).astype(F)
                py = (o[1] + ky.astype(F) * cs).astype(F)
                pz = (o[2] + kz.astype(F) * cs).astype(F)
                gx, gy, gz = np.meshgrid(px, py, pz, indexing="ij")  # z fastest: groups of 4 z
                xs.append(gx.ravel()), ys.append(gy.ravel()), zs.append(gz.ravel())
                ins.append(np.full(64, bool(side)))
        if not xs:
            e = np.zeros(0, F)
            return e, e, e, np.zeros(0, bool)
        return np.concatenate(xs), np.concatenate(ys), np.concatenate(zs), np.concatenate(ins)
