"""The run-time compiler's lifecycle through the C-ABI: a model, an option or the context itself
changed while kernels compile on a host thread.  A compile that is replaced finishes in the
background, a context waits for its compiles before it goes, and whatever serves meanwhile
(interpreter or kernels) gives the oracle's mesh bit for bit.  A cached code object may finish a
compile before the next call, so these tests assert outcomes, never that something was pending.
"""
import pytest

from gui_util import random_tree
from parity_util import assert_mesh_matches
from parsip_amd import gpu, gui, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def configs(oracle):
    """C1 (1 primitive, 32^3) and C2 (8 primitives, 128^3): model, cell size, the oracle's mesh."""
    out = {}
    for name in ("C1", "C2"):
        model, cs, _ = synth.make_config(name)
        out[name] = (model, cs, oracle.polygonize(model, cs, threads=8))
    return out


def _run_matches(p, cs, om):
    p.run(cs)
    assert_mesh_matches(p.download(), p.stats(), om)


def test_model_replaced_under_its_compile(configs):
    (m1, _, _), (m2, cs2, om2) = configs["C1"], configs["C2"]
    p = gpu.Polygonizer(0)
    try:
        p.set_model(m1, wait_jit=False)
        p.set_model(m2, wait_jit=False)
        _run_matches(p, cs2, om2)  # at once: the interpreter, or C2's kernels if they are in
        assert p.jit_wait() is True
        assert p.jit_tier == 1
        _run_matches(p, cs2, om2)
    finally:
        p.close()


def test_options_under_a_compile(configs):
    m2, cs2, om2 = configs["C2"]
    p = gpu.Polygonizer(0)
    try:
        p.set_model(m2, wait_jit=False)
        for mode in (2, 3, 1):
            p.set_option(gpu.OPT_JIT, mode)
        p.set_option(gpu.OPT_TREE_SPLIT, 1)
        p.set_option(gpu.OPT_TREE_SPLIT, 0)
        p.jit_wait()
        _run_matches(p, cs2, om2)
    finally:
        p.close()


def test_close_under_a_compile(configs):
    (m1, cs1, om1), (m2, _, _) = configs["C1"], configs["C2"]
    p = gpu.Polygonizer(0)
    p.set_model(m2, wait_jit=False)
    p.close()
    g = gpu.Group([0, 0])
    g.set_model(m2, wait_jit=False)
    g.close()
    e = gui.ParsipOptimized(0, jit=1)
    _, tree = gui.compact_blobtree(random_tree(41, n_prims=14))
    e.set_tree(tree)
    e.close()
    p = gpu.Polygonizer(0)
    try:
        p.set_model(m1)
        _run_matches(p, cs1, om1)
    finally:
        p.close()
