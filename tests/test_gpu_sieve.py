"""k_sieve ahead of S1 (PSGPU_OPT_SIEVE) on the device, C2-sized runs: with the sieve forced on
the mesh is the oracle's bit for bit, equals the mesh without it, and so do the per-MPU S1
decisions, counts and the run's counters -- through k_front and the separate launches, the tree
split, the interpreter, the baked tier, a ragged range, a group of 8 parts and graph replay."""
import numpy as np
import pytest

from parity_util import assert_bits_equal, assert_mesh_matches
from parsip_amd import gpu, synth
from sieve_util import Sieve, far_tree

pytestmark = pytest.mark.gpu

DEFAULTS = {gpu.OPT_JIT: 1, gpu.OPT_FRONT: 2, gpu.OPT_FUSED_SURFACE: 2, gpu.OPT_TREE_SPLIT: 0, gpu.OPT_CULLING: 1,
            gpu.OPT_GRAPH: 0, gpu.OPT_SIEVE: 0, gpu.OPT_SPLIT_MAX_QUEUED: 1024}
SEPARATE = {gpu.OPT_FRONT: 0, gpu.OPT_FUSED_SURFACE: 0}
BEGIN, END = 2 * 19 * 19 + 7 * 19 + 5, 6859 - (3 * 19 * 19 + 11 * 19 + 8)  # inside bricks, mid-row

# name -> (options, flags that must be set, flags that must not, MPU range, runs)
VARIANTS = {
    "front": ({gpu.OPT_FRONT: 1, gpu.OPT_TREE_SPLIT: 2, gpu.OPT_SPLIT_MAX_QUEUED: 0}, gpu.LAUNCH_FRONT, gpu.LAUNCH_TREE_SPLIT, None, 1),
    "separate": (SEPARATE, 0, gpu.LAUNCH_FRONT | gpu.LAUNCH_TREE_SPLIT, None, 1),
    "split": ({**SEPARATE, gpu.OPT_TREE_SPLIT: 1}, gpu.LAUNCH_TREE_SPLIT, gpu.LAUNCH_FRONT, None, 1),
    "front_split": ({gpu.OPT_FRONT: 1, gpu.OPT_TREE_SPLIT: 1}, gpu.LAUNCH_FRONT | gpu.LAUNCH_TREE_SPLIT, 0, None, 1),
    "interpreter": ({gpu.OPT_JIT: 0}, 0, gpu.LAUNCH_FRONT, None, 1),
    "baked": ({gpu.OPT_JIT: 2}, 0, 0, None, 1),
    "ragged": ({}, 0, 0, (BEGIN, END), 1),
    "ragged_separate": (SEPARATE, 0, gpu.LAUNCH_FRONT, (BEGIN, END), 1),
    "graph": ({gpu.OPT_GRAPH: 1}, 0, 0, None, 4),  # both counter sets captured, then replayed
}
INFO = ("ctMPUs", "ctPassedPrecheck", "ctSurfaceMPUs", "ctVertices", "ctTriangles", "firstOverflowMPU",
        "ctLaneEvals", "ctFieldMPUs")


@pytest.fixture(scope="module")
def c2(oracle):
    model, cs, _ = synth.make_config("C2")
    return model, cs, {None: oracle.polygonize(model, cs, threads=8),
                       (BEGIN, END): oracle.polygonize(model, cs, BEGIN, END, threads=8)}


def _set(poly, opts):
    for k, v in opts.items():
        poly.set_option(k, v)


def _run(poly, cs, rng, runs=1):
    for _ in range(runs):
        info = poly.run(cs, *(rng or ()))
    return info, poly.download(), poly.stats()


@pytest.mark.parametrize("name", list(VARIANTS))
def test_sieve_changes_no_bit(gpu_poly, c2, name):
    model, cs, om = c2
    opts, want, never, rng, runs = VARIANTS[name]
    try:
        _set(gpu_poly, {**DEFAULTS, **opts, gpu.OPT_SIEVE: 1})
        gpu_poly.set_model(model)
        info1, mesh1, st1 = _run(gpu_poly, cs, rng, runs)
        live = gpu_poly.live_bricks()
        gpu_poly.set_option(gpu.OPT_SIEVE, 0)
        info0, mesh0, st0 = _run(gpu_poly, cs, rng, runs)
    finally:
        _set(gpu_poly, DEFAULTS)
    assert info1.launchFlags & gpu.LAUNCH_SIEVE and not info0.launchFlags & gpu.LAUNCH_SIEVE
    for info in (info0, info1):
        assert info.launchFlags & want == want and not info.launchFlags & never, (name, info.launchFlags)
    assert_mesh_matches(mesh1, st1, om[rng])
    for f in INFO:
        assert getattr(info1, f) == getattr(info0, f), f
    np.testing.assert_array_equal(st1, st0)  # passed, evaluations and counts per MPU
    for a in ("pos", "nrm", "col"):
        assert_bits_equal(getattr(mesh1, a), getattr(mesh0, a), a)
    np.testing.assert_array_equal(mesh1.tris, mesh0.tris)
    # the list is the CPU program's live set, in any order, each brick once
    want_live = Sieve(model, cs, "gpu_c2").live_set(*(rng or (0, None)))
    assert len(live) == len(want_live) and {tuple(int(x) for x in b) for b in live} == want_live


def test_culling_off_takes_no_sieve(gpu_poly, c2):
    model, cs, om = c2
    try:
        _set(gpu_poly, {**DEFAULTS, gpu.OPT_SIEVE: 1, gpu.OPT_CULLING: 0})
        gpu_poly.set_model(model)
        info, mesh, st = _run(gpu_poly, cs, None)
        assert len(gpu_poly.live_bricks()) == 0
    finally:
        _set(gpu_poly, DEFAULTS)
    assert not info.launchFlags & gpu.LAUNCH_SIEVE
    assert_mesh_matches(mesh, st, om[None])


def test_group_of_eight_parts(c2):
    model, cs, om = c2
    g = gpu.Group([0] * 8)
    try:
        g.set_option(gpu.GROUP_OPT_MIN_PART_MPUS, 0)
        g.set_option(gpu.OPT_SIEVE, 1)
        g.set_model(model)
        info, parts = g.run(cs)
        mesh = g.download()
        assert len(parts) == 8 and all(p.info.launchFlags & gpu.LAUNCH_SIEVE for p in parts if p.info.ctMPUs)
        assert sum(1 for p in parts if p.info.ctMPUs) > 1
    finally:
        g.close()
    o = om[None]
    assert (info.ctVertices, info.ctTriangles) == (len(o.pos), len(o.tris))
    assert_bits_equal(mesh.pos, o.pos, "positions")
    assert_bits_equal(mesh.nrm, o.nrm, "normals")
    assert_bits_equal(mesh.col, o.col, "colours")
    np.testing.assert_array_equal(mesh.local_tris(), o.tris)
    assert info.ctPassedPrecheck == int(np.count_nonzero(o.stats[:, 0]))


def test_plan_takes_the_sieve_only_among_other_runs(c2):
    """Option 2 (the plan decides): four contexts with runs in flight take the sieve (all but the
    one enqueued while the device was idle); a context alone does not.  The default is 0 (the
    sieve measured slower than S1 without it, DESIGN.md section 4 "Round 12"): no sieve."""
    model, cs, om = c2
    polys = [gpu.Polygonizer(0) for _ in range(4)]
    try:
        for p in polys:
            p.set_model(model)
        for p in polys:
            p.polygonize(cs)
        assert not any(p.finish().launchFlags & gpu.LAUNCH_SIEVE for p in polys)
        for p in polys:
            p.set_option(gpu.OPT_SIEVE, 2)
        for p in polys:  # a first round sizes the grids
            p.run(cs)
        for p in polys:
            p.polygonize(cs)
        infos = [p.finish() for p in polys]
        assert all(i.launchFlags & gpu.LAUNCH_SIEVE for i in infos[1:]), [i.launchFlags for i in infos]
        for p in polys:
            assert_mesh_matches(p.download(), p.stats(), om[None])
        lone = polys[0].run(cs)
        assert not lone.launchFlags & gpu.LAUNCH_SIEVE
        assert_mesh_matches(polys[0].download(), polys[0].stats(), om[None])
    finally:
        for p in polys:
            p.close()


def test_every_brick_dead_gives_an_empty_mesh(gpu_poly, oracle):
    model, cs = far_tree(), synth.make_config("C2")[1]
    om = oracle.polygonize(model, cs, threads=8)
    assert len(om.pos) == 0
    try:
        _set(gpu_poly, {**DEFAULTS, gpu.OPT_SIEVE: 1})
        gpu_poly.set_model(model)
        info, mesh, st = _run(gpu_poly, cs, None)
        assert len(gpu_poly.live_bricks()) == 0
    finally:
        _set(gpu_poly, DEFAULTS)
    assert info.launchFlags & gpu.LAUNCH_SIEVE
    assert (info.ctVertices, info.ctTriangles, info.ctPassedPrecheck) == (0, 0, 0)
    assert_mesh_matches(mesh, st, om)
