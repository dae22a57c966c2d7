"""The op-inside masks on the device (PSGPU_OPT_OP_INSIDE; k_precheck makes them, the generated
walks skip the op-box pruning tests they cover): with the option on the mesh is the oracle's bit
for bit and equal to the mesh with the option off, and the masks the run used equal the CPU
program's (tests/cpp/op_inside_check.cpp), so the skip path really ran -- for every input of
op_inside_util.CASES through the default launches, and once through each kernel variant that
carries the masks."""
import numpy as np
import pytest

from parsip_amd import gpu, soa
from parity_util import assert_bits_equal, assert_mesh_matches
import op_inside_util as U

pytestmark = pytest.mark.gpu

DEFAULTS = {gpu.OPT_JIT: 1, gpu.OPT_FRONT: 2, gpu.OPT_FUSED_SURFACE: 2, gpu.OPT_TREE_SPLIT: 0, gpu.OPT_VERTEX_WIDE: 2,
            gpu.OPT_FINISH_QUAD: 2, gpu.OPT_OP_INSIDE: 1}
SEPARATE = {gpu.OPT_FRONT: 0, gpu.OPT_FUSED_SURFACE: 0}
# name -> (options, launch flags that must be set, launch flags that must be clear)
MODES = {
    "default": ({}, 0, 0),
    "separate": (SEPARATE, 0, gpu.LAUNCH_FRONT | gpu.LAUNCH_SURFACE | gpu.LAUNCH_TREE_SPLIT),
    "front": ({gpu.OPT_FRONT: 1, gpu.OPT_FUSED_SURFACE: 0}, gpu.LAUNCH_FRONT, gpu.LAUNCH_SURFACE),
    "surface": ({gpu.OPT_FRONT: 0, gpu.OPT_FUSED_SURFACE: 1}, gpu.LAUNCH_SURFACE, gpu.LAUNCH_FRONT),
    "split": ({**SEPARATE, gpu.OPT_TREE_SPLIT: 1}, gpu.LAUNCH_TREE_SPLIT, gpu.LAUNCH_FRONT),
    "front_split": ({gpu.OPT_FRONT: 1, gpu.OPT_FUSED_SURFACE: 0, gpu.OPT_TREE_SPLIT: 1},
                    gpu.LAUNCH_FRONT | gpu.LAUNCH_TREE_SPLIT, 0),
    "wide": ({**SEPARATE, gpu.OPT_VERTEX_WIDE: 1, gpu.OPT_FINISH_QUAD: 0}, 0, gpu.LAUNCH_SURFACE),
    "pair": ({**SEPARATE, gpu.OPT_VERTEX_WIDE: 0, gpu.OPT_FINISH_QUAD: 3}, 0, gpu.LAUNCH_SURFACE),
    "quad": ({**SEPARATE, gpu.OPT_VERTEX_WIDE: 0, gpu.OPT_FINISH_QUAD: 1}, 0, gpu.LAUNCH_SURFACE),
    "baked": ({gpu.OPT_JIT: 2}, 0, 0),
}
# every input through the default launches; each variant on C3 and on a chain (the tree split on
# C3 and C5: a chain's root has a primitive child, which the split does not take)
RUNS = [("default", n) for n in U.CASES] + [(m, n) for m in MODES if m != "default"
                                            for n in (("C3_64", "C5_64") if "split" in m else ("C3_64", "chain7"))]


@pytest.fixture(scope="module")
def oracle_meshes(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            model, cs = U.make_case(name)
            cache[name] = oracle.polygonize(model, cs, threads=8)
        return cache[name]
    return get


def check_masks(name, model, queued, masks, on):
    want = U.cpu_masks(name)
    assert queued.any() and masks.shape == (len(want), 4)
    assert not masks[~queued].any()
    if on:
        np.testing.assert_array_equal(masks[queued, 2:], want[queued], err_msg="op-inside masks")
        deep = U.op_depths(model) > 3
        assert U.mask_bits(masks[queued, 2:], model.ct_ops)[:, deep].any(), "no deep op's test was skipped"
    else:
        assert not masks[:, 2:].any()


@pytest.mark.parametrize("mode,name", RUNS)
def test_mesh_and_masks(gpu_poly, oracle_meshes, mode, name):
    model, cs = U.make_case(name)
    om = oracle_meshes(name)
    opts, must, must_not = MODES[mode]
    try:
        for k, v in {**DEFAULTS, **opts}.items():
            gpu_poly.set_option(k, v)
        gpu_poly.set_model(model)
        gpu_poly.jit_wait()
        assert gpu_poly.jit_active
        info = gpu_poly.run(cs)
        assert (info.launchFlags & must) == must and not (info.launchFlags & must_not), (mode, info.launchFlags)
        on = gpu_poly.download()
        assert_mesh_matches(on, gpu_poly.stats(), om)
        check_masks(name, model, *gpu_poly.mpu_masks(), True)
        gpu_poly.set_option(gpu.OPT_OP_INSIDE, 0)
        gpu_poly.run(cs)
        off = gpu_poly.download()
        check_masks(name, model, *gpu_poly.mpu_masks(), False)
        for a, b, what in ((on.pos, off.pos, "positions"), (on.nrm, off.nrm, "normals"), (on.col, off.col, "colours")):
            assert_bits_equal(a, b, f"{what}, option on vs off")
        np.testing.assert_array_equal(on.tris, off.tris)
        np.testing.assert_array_equal(on.vertex_offsets, off.vertex_offsets)
    finally:
        for k, v in DEFAULTS.items():
            gpu_poly.set_option(k, v)


def test_group_of_eight_parts(oracle_meshes):
    """C3 at 64^3 cells as 8 ranges on one device: the reassembled mesh is the oracle's, and each
    part's masks are the CPU program's for its range."""
    name = "C3_64"
    model, cs = U.make_case(name)
    om = oracle_meshes(name)
    want = U.cpu_masks(name)
    L = gpu.load()
    g = gpu.Group([0] * 8)
    try:
        g.set_model(model)
        info, parts = g.run(cs)
        mesh = g.download()
        assert_bits_equal(mesh.pos, om.pos, "positions")
        assert_bits_equal(mesh.nrm, om.nrm, "normals")
        assert_bits_equal(mesh.col, om.col, "colours")
        np.testing.assert_array_equal(mesh.local_tris(), om.tris)
        np.testing.assert_array_equal(mesh.vertex_offsets, om.vertex_offsets)
        seen = 0
        for p, part in enumerate(parts):
            n = part.mpuEnd - part.mpuBegin
            queued, masks = np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 4), np.uint64)
            assert L.psgpu_mpu_masks(g.context_ptr(p), queued.ctypes.data, masks.ctypes.data, len(queued)) == soa.RET_SUCCESS
            q = queued[:n].astype(bool)
            np.testing.assert_array_equal(masks[:n][q, 2:], want[part.mpuBegin:part.mpuEnd][q], err_msg=f"part {p}")
            seen += int(masks[:n][q, 2:].any(1).sum())
        assert parts[0].mpuBegin == 0 and parts[-1].mpuEnd == info.ctMPUs == len(want) and seen > 0
    finally:
        g.close()
