"""S2 walks only the octants S1's field bounds left undecided (DESIGN.md §4 "S2 octants"), on the
device: through k_front, the separate launches, the interpreter, the baked tier, the tree split
(which ignores the verdicts but reads the wider queue entry), k_surface, without bounds and with
the ablation bit (every octant walked) the mesh is the oracle's bit for bit (parity_util); the
counters ctPassedPrecheck and ctSurfaceMPUs are the oracle's, ctFieldMPUs is the host model's count
of queued MPUs and not above the figure recorded in tests/golden/cullbound_counts.json; the 16
verdict bits of every MPU's queue entry are the host model's, MPU by MPU
(tests/cpp/s2_octants_check.cpp; the tree-split S1's too, which no kernel reads); and the device's
count of S2 passes is the host model's, 2 per queued MPU with the ablation bit, none for the tree
split.  Every input takes every path: 46 inputs x 8 paths, about a second each."""
import json

import numpy as np
import pytest

import cullbound_util as U
import s2_octants_util as S
from parity_util import assert_mesh_matches
from parsip_amd import gpu

pytestmark = pytest.mark.gpu

DEFAULTS = {gpu.OPT_JIT: 1, gpu.OPT_FRONT: 2, gpu.OPT_FUSED_SURFACE: 2, gpu.OPT_TREE_SPLIT: 0, gpu.OPT_CULLING: 1,
            gpu.OPT_BOUND: 1, gpu.OPT_DEBUG: 0}
SEPARATE = {gpu.OPT_FRONT: 0, gpu.OPT_FUSED_SURFACE: 0}
COUNT = gpu.DEBUG_S2_COUNT_PASSES
# name -> (options, launch flags that must be set, launch flags that must be clear)
PATHS = {
    "front": ({gpu.OPT_FRONT: 1, gpu.OPT_FUSED_SURFACE: 0}, gpu.LAUNCH_FRONT, gpu.LAUNCH_SURFACE),
    "separate": (SEPARATE, 0, gpu.LAUNCH_FRONT | gpu.LAUNCH_SURFACE | gpu.LAUNCH_TREE_SPLIT),
    "interpreter": ({**SEPARATE, gpu.OPT_JIT: 0}, 0, gpu.LAUNCH_FRONT | gpu.LAUNCH_SURFACE | gpu.LAUNCH_TREE_SPLIT),
    "baked": ({gpu.OPT_JIT: 2}, 0, 0),
    "split": ({**SEPARATE, gpu.OPT_TREE_SPLIT: 1}, gpu.LAUNCH_TREE_SPLIT, gpu.LAUNCH_FRONT),
    "surface": ({gpu.OPT_FRONT: 0, gpu.OPT_FUSED_SURFACE: 1}, gpu.LAUNCH_SURFACE, gpu.LAUNCH_FRONT),
    "nobound": ({gpu.OPT_FRONT: 1, gpu.OPT_BOUND: 0}, gpu.LAUNCH_FRONT, 0),
    "ablation": ({gpu.OPT_FRONT: 1, gpu.OPT_DEBUG: COUNT | gpu.DEBUG_S2_ALL_OCTANTS}, gpu.LAUNCH_FRONT, 0),
}
# every case through every path (a tree the split does not apply to takes the separate launches there)
RUNS = [(n, p) for n in S.CASES for p in PATHS]
TIER = {"interpreter": 0, "baked": 2}  # the kernels that must run (jit_tier); every other path: 1

_ORACLE, _MODEL = {}, {}


@pytest.fixture(scope="module")
def recorded_field_mpus():
    with open(U.GOLDEN) as f:
        return json.load(f)["parent_ctFieldMPUs"]


def reference(oracle, name, bound):
    """The oracle's mesh of a case and the host model's verdicts on it, each made once."""
    model, cs = S.make_case(name)
    if name not in _ORACLE:
        _ORACLE[name] = oracle.polygonize(model, cs, threads=8)
    if (name, bound) not in _MODEL:
        _MODEL[name, bound] = S.Verdicts(model, cs, _ORACLE[name].stats[:, 0], f"{name}_{int(bound)}", bound=bound)
    return _ORACLE[name], _MODEL[name, bound]


@pytest.mark.parametrize("name,path", RUNS)
def test_mesh_counters_and_passes(gpu_poly, oracle, recorded_field_mpus, name, path):
    model, cs = S.make_case(name)
    opts, must, must_not = PATHS[path]
    # the interpreter's bound() proves nothing: its entries carry no verdict
    om, v = reference(oracle, name, bound=path not in ("nobound", "interpreter"))
    try:
        for k, val in {**DEFAULTS, gpu.OPT_DEBUG: COUNT, **opts}.items():
            gpu_poly.set_option(k, val)
        gpu_poly.set_model(model)
        gpu_poly.jit_wait()
        tier = gpu_poly.jit_tier
        info = gpu_poly.run(cs)
        mesh, stats, passes = gpu_poly.download(), gpu_poly.stats(), gpu_poly.s2_passes()
        words = gpu_poly.mpu_octants()
    finally:
        for k, val in DEFAULTS.items():
            gpu_poly.set_option(k, val)
    assert tier == TIER.get(path, 1), (path, tier)
    if not S.tree_splits(model):
        must &= ~gpu.LAUNCH_TREE_SPLIT
    assert (info.launchFlags & must) == must and not (info.launchFlags & must_not), (path, info.launchFlags)
    assert_mesh_matches(mesh, stats, om)
    passed, surface = int(np.count_nonzero(om.stats[:, 0])), int(np.count_nonzero(om.stats[:, 3]))
    queued = int(np.count_nonzero(v.queued))
    print(f"{name} {path}: passed S1 {info.ctPassedPrecheck}, S2-evaluated {info.ctFieldMPUs} (model {queued}), "
          f"surface {info.ctSurfaceMPUs}, S2 passes {passes} (model {int(v.passes.sum())}, all octants {2 * queued})")
    assert info.ctPassedPrecheck == passed
    assert info.ctSurfaceMPUs == surface
    assert info.ctFieldMPUs == queued
    if name in recorded_field_mpus and path in recorded_field_mpus[name]:
        assert info.ctFieldMPUs <= recorded_field_mpus[name][path]
    np.testing.assert_array_equal(words, v.entry_words(), err_msg="the queue entries' octant verdicts, per MPU")
    if info.launchFlags & gpu.LAUNCH_TREE_SPLIT:
        assert passes == 0
    elif path == "ablation":
        assert passes == 2 * queued
    else:
        assert passes == int(v.passes.sum())


def test_c2_walks_fewer_passes_than_all_octants(gpu_poly, oracle):
    """The verdicts are in use: on C2 the device walks the model's 673 passes, not 2 x 519."""
    model, cs = S.make_case("C2")
    _, v = reference(oracle, "C2", bound=True)
    try:
        gpu_poly.set_option(gpu.OPT_DEBUG, COUNT)
        gpu_poly.set_model(model)
        gpu_poly.jit_wait()
        gpu_poly.run(cs)
        passes = gpu_poly.s2_passes()
    finally:
        gpu_poly.set_option(gpu.OPT_DEBUG, 0)
    assert passes == int(v.passes.sum()) < 2 * int(np.count_nonzero(v.queued))
