"""The named inputs of the weld tests (tests/test_weld.py, tests/test_gpu_weld.py,
tests/golden/make_weld_counts.py) and the comparisons they share."""
import json
import os

import numpy as np

from parsip_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weld_counts.json")

# name -> (kind, which, cellsize, MPU range); the power-of-two cell sizes (C1, C2: 1/16) round
# every corner alike from both sides of a seam, the others do not
CASES = {
    "C1": ("config", "C1", None, None),
    "C2": ("config", "C2", None, None),
    "rand3_0.071": ("random", 3, 0.071, None),
    "rand4_0.123457": ("random", 4, 0.123457, None),
    "rand1_0.13": ("random", 1, 0.13, None),
    "rand3_0.071_mpus_243_486": ("random", 3, 0.071, (243, 486)),
    # the same closed surface in a box that is no cube: a (6, 7, 5) lattice (tests/aniso_util.py)
    "rand3_0.071_box_6x7x5": ("boxed", 3, 0.071, None),
}
# Inputs for the branches of the shared mesh stages (psgpu_mesh_stages.h), kept out of CASES:
# they have no entry in the golden count files, their counts stand here.
# MPU prefix ranges of rand1_0.13 whose run vertices V, triangles T and welded vertices Vw
# take every residue mod 4 between them (the 16-byte loads' scalar tails; [0, 26) is smaller
# than one wave): name -> (V, T, Vw)
TAIL_COUNTS = {
    "rand1_0.13_mpus_0_26": (60, 91, 60),
    "rand1_0.13_mpus_0_30": (73, 104, 73),
    "rand1_0.13_mpus_0_32": (303, 461, 276),
    "rand1_0.13_mpus_0_54": (1432, 2238, 1222),
    "rand1_0.13_mpus_0_85": (2586, 3960, 2051),
}
# C2's model at half its cell size: more than 256 blocks of 256 in each of the weld's, the
# shells' and the filter's scans (k_weld_scan's carry loop): (MPUs, V, T, Vw)
SCAN_NAME = "C2_0.03125"
SCAN_COUNTS = (50653, 126580, 194092, 97292)
STAGE_CASES = {name: ("random", 1, 0.13, (0, int(name.rsplit("_", 1)[1]))) for name in TAIL_COUNTS}
STAGE_CASES[SCAN_NAME] = ("config", "C2", 0.03125, None)

BOXED_NAME = "rand3_0.071_box_6x7x5"
BOX_LO, BOX_HI = (-1.35, -1.10, -1.03), (1.17, 1.95, 1.02)


def make_case(name):
    """(model, cellsize, (mpu_begin, mpu_end or None))."""
    kind, which, cs, rng = CASES[name] if name in CASES else STAGE_CASES[name]
    if kind == "config":
        model, own, _ = synth.make_config(which)
        cs = own if cs is None else cs
    else:
        model = synth.random_model(which, 6)
    if kind == "boxed":
        model.prims["bboxLo"][0] = BOX_LO
        model.prims["bboxHi"][0] = BOX_HI
    return model, cs, rng or (0, None)


def golden_counts():
    with open(GOLDEN) as f:
        return json.load(f)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_contract(mesh_pos, mesh_nrm, mesh_col, mesh_tris, w, vertex_map):
    """The weld's contract on any (input mesh, welded mesh, map): the map is onto [0, Vw), first
    occurrences increase, welded attributes are the first occurrences' bits, and the triangles
    are the input's through the map, none dropped."""
    vm = np.asarray(vertex_map).astype(np.int64)
    nw = len(w.pos)
    assert len(vm) == len(mesh_pos)
    if len(vm) == 0:
        assert nw == 0 and len(w.tris) == 0
        return
    assert vm.min() == 0 and vm.max() == nw - 1
    ids, first = np.unique(vm, return_index=True)
    assert np.array_equal(ids, np.arange(nw))            # onto
    assert (np.diff(first) > 0).all()                    # ordered by first occurrence
    for got, src in ((w.pos, mesh_pos), (w.nrm, mesh_nrm), (w.col, mesh_col)):
        assert np.array_equal(u32(got), u32(src)[first])
    assert np.array_equal(np.asarray(w.tris).astype(np.int64), vm[np.asarray(mesh_tris).astype(np.int64)])
