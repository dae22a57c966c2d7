"""The box bounds of the culling masks and of the S1 field proofs on the device (cull_one with
the box's half-extents, prim_interval: psgpu_model.h): the mesh is the oracle's bit for bit
(parity_util) through k_front, the separate launches, the tree split, the interpreter, the baked
tier and k_surface; the counters ctPassedPrecheck and ctSurfaceMPUs are the oracle's; and
ctFieldMPUs (the MPUs S2 evaluates) is not above what the sphere forms gave for the same input
(recorded once from the commit before the box forms, tests/golden/cullbound_counts.json)."""
import json

import numpy as np
import pytest

import aniso_util
import cullbound_util as U
from parity_util import assert_mesh_matches
from parsip_amd import gpu, synth
from parsip_amd.soa import NodeType
from sieve_util import fuzz_tree

pytestmark = pytest.mark.gpu

DEFAULTS = {gpu.OPT_JIT: 1, gpu.OPT_FRONT: 2, gpu.OPT_FUSED_SURFACE: 2, gpu.OPT_TREE_SPLIT: 0, gpu.OPT_CULLING: 1,
            gpu.OPT_BOUND: 1}
SEPARATE = {gpu.OPT_FRONT: 0, gpu.OPT_FUSED_SURFACE: 0}
# name -> (options, launch flags that must be set, launch flags that must be clear)
PATHS = {
    "front": ({gpu.OPT_FRONT: 1, gpu.OPT_FUSED_SURFACE: 0}, gpu.LAUNCH_FRONT, gpu.LAUNCH_SURFACE),
    "separate": (SEPARATE, 0, gpu.LAUNCH_FRONT | gpu.LAUNCH_SURFACE | gpu.LAUNCH_TREE_SPLIT),
    "split": ({**SEPARATE, gpu.OPT_TREE_SPLIT: 1}, gpu.LAUNCH_TREE_SPLIT, gpu.LAUNCH_FRONT),
    "interpreter": ({**SEPARATE, gpu.OPT_JIT: 0}, 0, gpu.LAUNCH_FRONT | gpu.LAUNCH_SURFACE | gpu.LAUNCH_TREE_SPLIT),
    "baked": ({gpu.OPT_JIT: 2}, 0, 0),
    "surface": ({gpu.OPT_FRONT: 0, gpu.OPT_FUSED_SURFACE: 1}, gpu.LAUNCH_SURFACE, gpu.LAUNCH_FRONT),
}
ONLY = {"cubes": NodeType.CUBE, "cylinders": NodeType.CYLINDER, "lines": NodeType.LINE}


def _c3_538():
    model = aniso_util.boxed(synth.make_config("C3")[0],
                             *aniso_util.box_for((5, 3, 8), aniso_util.FIRST, aniso_util.CS))
    return model, aniso_util.CS


# name -> () -> (model, cell size): C2, C3 at 64^3 cells, C3's tree in a 5x3x8 lattice, trees of
# one primitive type whose primitives touch MPU faces, the fuzz trees at 32^3 cells
CASES = {"C2": lambda: synth.make_config("C2")[:2], "C3_64": lambda: U.coarse("C3", 64), "C3_5x3x8": _c3_538}
CASES.update({f"only_{k}": (lambda t=t, i=i: (U.only_tree(t, 4.0 / 64, 40 + i), 4.0 / 64))
              for i, (k, t) in enumerate(ONLY.items())})
CASES.update({f"fuzz{s}": (lambda s=s: (fuzz_tree(s), 4.0 / 32)) for s in range(20)})
# every named case through every path; fuzz tree s through path s mod 6 (whatever launches its
# tree allows: a root with a primitive child takes no split)
RUNS = [(n, p) for n in CASES if not n.startswith("fuzz") for p in PATHS] + \
       [(f"fuzz{s}", list(PATHS)[s % 6]) for s in range(20)]

_MODELS, _ORACLE = {}, {}


def make_case(name):
    if name not in _MODELS:
        _MODELS[name] = CASES[name]()
    return _MODELS[name]


def run_case(poly, name, path):
    """One run of a case through a path on the context: (info, mesh, stats)."""
    model, cs = make_case(name)
    try:
        for k, v in {**DEFAULTS, **PATHS[path][0]}.items():
            poly.set_option(k, v)
        poly.set_model(model)
        poly.jit_wait()
        info = poly.run(cs)
        return info, poly.download(), poly.stats()
    finally:
        for k, v in DEFAULTS.items():
            poly.set_option(k, v)


@pytest.fixture(scope="module")
def parent_field_mpus():
    with open(U.GOLDEN) as f:
        return json.load(f)["parent_ctFieldMPUs"]


@pytest.mark.parametrize("name,path", RUNS)
def test_mesh_and_counters(gpu_poly, oracle, parent_field_mpus, name, path):
    model, cs = make_case(name)
    if name not in _ORACLE:
        _ORACLE[name] = oracle.polygonize(model, cs, threads=8)
    om = _ORACLE[name]
    info, mesh, stats = run_case(gpu_poly, name, path)
    _, must, must_not = PATHS[path]
    if not name.startswith("fuzz"):
        assert (info.launchFlags & must) == must and not (info.launchFlags & must_not), (path, info.launchFlags)
    assert_mesh_matches(mesh, stats, om)
    passed, surface = int(np.count_nonzero(om.stats[:, 0])), int(np.count_nonzero(om.stats[:, 3]))
    print(f"{name} {path}: passed S1 {info.ctPassedPrecheck}, S2-evaluated {info.ctFieldMPUs} "
          f"(before: {parent_field_mpus[name][path]}), surface {info.ctSurfaceMPUs}")
    assert info.ctPassedPrecheck == passed
    assert info.ctSurfaceMPUs == surface
    assert surface <= info.ctFieldMPUs <= passed
    assert info.ctFieldMPUs <= parent_field_mpus[name][path]


def test_box_forms_prove_more_on_c3(gpu_poly, parent_field_mpus):
    """The tighter intervals are in use: C3 at 64^3 cells sends fewer MPUs to S2 than before."""
    info, _, _ = run_case(gpu_poly, "C3_64", "front")
    assert info.ctFieldMPUs < parent_field_mpus["C3_64"]["front"]
