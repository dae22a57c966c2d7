"""Device memory (parsip_amd/csrc/psgpu_buf.h; DESIGN.md §3 "Device memory"): every context,
group and compatibility context gives back exactly the device bytes it took, on the paths that
grow, restart and hand buffers from one device part to another.

gpu.device_bytes() counts the library's own allocations of this process, so the comparisons are
exact on a card that other processes use; contexts of other modules' fixtures stay as they are
between a test's two readings.  The paths on which an allocation fails (a reserve that fails,
the second or third buffer of the two field_values) would need the card's memory exhausted:
they are checked by reading the code."""
import numpy as np
import pytest

from gui_util import assert_gui_mesh_equal, random_tree
from parsip_amd import gpu, gui
from test_gpu_weld import weld_bytes
from test_gui import _pcm_pair
from weld_util import make_case

pytestmark = pytest.mark.gpu

NAME = "rand3_0.071"  # about 4,000 vertices


def run_case(p):
    model, cs, (b, e) = make_case(NAME)
    p.set_model(model)
    return p.run(cs, b, e)


def test_context_returns_every_byte():
    assert gpu.device_count() > 0, "no HIP device visible: GPU tests must run on an MI355X"
    base = gpu.device_bytes()
    p = gpu.Polygonizer(0)
    try:
        p.set_option(gpu.OPT_CAPACITY, 64)
        info = run_case(p)
        assert info.launchFlags & gpu.LAUNCH_RERUN  # the buffers grew
        w = p.weld()
        assert w.info.ctVertices > 0
        assert p.weld_shells().info["ctShells"] > 0
        xyz = np.random.default_rng(3).uniform(-1, 1, size=(64, 3)).astype(np.float32)
        assert len(p.field_values(xyz)) == 64
        assert gpu.device_bytes() > base
    finally:
        p.close()
    assert gpu.device_bytes() == base


def test_capacity_restart_frees_and_reruns():
    base = gpu.device_bytes()
    p = gpu.Polygonizer(0)
    try:
        run_case(p)
        want = weld_bytes(p.weld())
        held = gpu.device_bytes()
        p.set_option(gpu.OPT_CAPACITY, 64)
        assert gpu.device_bytes() < held
        run_case(p)
        assert weld_bytes(p.weld()) == want
    finally:
        p.close()
    assert gpu.device_bytes() == base


def test_stamps_and_spans_come_and_go():
    base = gpu.device_bytes()
    p = gpu.Polygonizer(0)
    try:
        at = gpu.device_bytes()
        p.set_option(gpu.OPT_STAMPS, 256)
        with_stamps = gpu.device_bytes()
        assert with_stamps > at
        p.set_option(gpu.OPT_SPANS, 4)
        with_both = gpu.device_bytes()
        assert with_both > with_stamps
        p.set_option(gpu.OPT_STAMPS, 128)  # a smaller buffer replaces the old one
        assert at < gpu.device_bytes() < with_both
        p.set_option(gpu.OPT_SPANS, 0)
        p.set_option(gpu.OPT_STAMPS, 0)
        assert gpu.device_bytes() == at
    finally:
        p.close()
    assert gpu.device_bytes() == base


def test_group_on_one_device_returns_every_byte():
    base = gpu.device_bytes()
    g = gpu.Group([0] * 3)
    try:
        model, cs, _ = make_case(NAME)
        g.set_model(model)
        g.run(cs)
        first = weld_bytes(g.weld(dst_part=0))
        assert g.weld_shells().info["ctShells"] > 0
        second = weld_bytes(g.weld(dst_part=2))  # the gather and the weld move to another part
        assert second == first
        assert gpu.device_bytes() > base
    finally:
        g.close()
    assert gpu.device_bytes() == base


def test_group_gather_and_weld_move_between_parts_on_live_streams():
    """The group's gathered mesh and its weld are each torn down and rebuilt on another part while
    the gather stream and the timing events are in use: gather and timed weld on part 0, shells,
    the weld again on part 1 (same bytes), the gather back on part 0, destroy.  Two devices where
    there are two, else two parts on one."""
    base = gpu.device_bytes()
    g = gpu.Group([0, 1] if gpu.device_count() > 1 else [0, 0])
    try:
        model, cs, _ = make_case(NAME)
        g.set_option(gpu.OPT_KERNEL_TIMING, 1)
        g.set_model(model)
        info, _ = g.run(cs)
        assert g.gather(0).pos
        first = g.weld(dst_part=0)
        assert first.info.ctInputVertices == info.ctVertices > 0
        assert g.weld_times()["group weld total"] > 0
        assert g.weld_shells().info["ctShells"] > 0
        assert weld_bytes(g.weld(dst_part=1)) == weld_bytes(first)
        assert g.weld_times()["group weld total"] > 0
        assert g.gather(0).pos
        assert gpu.device_bytes() > base
    finally:
        g.close()
    assert gpu.device_bytes() == base


def test_compat_context_returns_every_byte():
    base = gpu.device_bytes()
    _, small = gui.compact_blobtree(_pcm_pair())
    code, other = gui.compact_blobtree(random_tree(1))
    assert code == 0
    p = gui.ParsipOptimized(0, jit=0)
    try:
        p.setup(small, None, 0, 0.04)
        assert p.run().ctVertices > 0
        xyz = np.random.default_rng(4).uniform(*small.root_octree, size=(64, 3)).astype(np.float32)
        assert len(p.field_values(xyz)[0]) == 64
        p.setup(other, None, 0, 0.06)
        p.run()
        got = p.exportMesh()
        assert gpu.device_bytes() > base
    finally:
        p.close()
    assert gpu.device_bytes() == base
    q = gui.ParsipOptimized(0, jit=0)
    try:
        q.setup(other, None, 0, 0.06)
        q.run()
        assert_gui_mesh_equal(got, q.exportMesh(), "second tree")
    finally:
        q.close()
    assert gpu.device_bytes() == base


def test_ten_cycles_end_where_they_began():
    base = gpu.device_bytes()
    for _ in range(10):
        p = gpu.Polygonizer(0)
        try:
            run_case(p)
            assert p.weld().info.ctVertices > 0
        finally:
            p.close()
    assert gpu.device_bytes() == base
