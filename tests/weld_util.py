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
BOXED_NAME = "rand3_0.071_box_6x7x5"
BOX_LO, BOX_HI = (-1.35, -1.10, -1.03), (1.17, 1.95, 1.02)


def make_case(name):
    """(model, cellsize, (mpu_begin, mpu_end or None))."""
    kind, which, cs, rng = CASES[name]
    if kind == "config":
        model, cs, _ = synth.make_config(which)
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
