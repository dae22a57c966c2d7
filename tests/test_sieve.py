"""k_sieve's decision on the CPU: tests/cpp/sieve_check.cpp compiles brick_box, the culled test
and the root-zero set from psgpu_model.h as a plain C++ program (sieve_util.py).  Every brick it
calls dead (every primitive the root needs is culled over the brick's S1 corner box) must have
no MPU that passes S1 in the oracle: the sieve then writes what S1 would have."""
import numpy as np
import pytest

from parsip_amd import soa, synth
from sieve_util import Sieve, disc_tree, far_tree, fuzz_tree, ricci_tree

F = np.float32


def _coarse(name, cells):
    model, cs, n = synth.make_config(name)
    return model, float(F(cs * n / cells))


def _ragged_c2():
    model, cs, _ = synth.make_config("C2")  # 19^3 MPUs: begins and ends inside a brick, mid-row
    return model, cs, 2 * 19 * 19 + 7 * 19 + 5, 6859 - (3 * 19 * 19 + 11 * 19 + 8)


# name -> (model, cellsize, begin, end)
CASES = {
    "C1": lambda: synth.make_config("C1")[:2] + (0, None),
    "C2": lambda: synth.make_config("C2")[:2] + (0, None),
    "C2_0.0713": lambda: (synth.make_config("C2")[0], 0.0713, 0, None),
    "C2_ragged": _ragged_c2,
    "C3_64": lambda: _coarse("C3", 64) + (0, None),
}


def check_dead_bricks(oracle, tag, model, cs, begin=0, end=None):
    sv = Sieve(model, cs, tag)
    assert sv.agree == 1, "the image's root-zero set is not the rule's"
    n = int(np.prod(sv.dims))
    end = n if end is None else end
    om = oracle.polygonize(model, cs, begin, end, threads=8, keep=False)
    assert len(om.stats) == end - begin
    dead = sv.mpu_dead()[begin:end]
    passed = om.stats[:, 0] != 0
    bad = np.flatnonzero(dead & passed)
    assert len(bad) == 0, f"{tag}: {len(bad)} MPUs pass S1 inside a dead brick, first {begin + int(bad[0])}"
    return sv, int(np.count_nonzero(dead)), passed


@pytest.mark.parametrize("name", list(CASES))
def test_dead_bricks_have_no_s1_survivor(oracle, name):
    model, cs, begin, end = CASES[name]()
    sv, dead_mpus, passed = check_dead_bricks(oracle, name, model, cs, begin, end)
    dead, bricks = int(np.count_nonzero(sv.dead)), int(sv.dead.size)
    print(f"{name}: {dead} of {bricks} bricks dead, {dead_mpus} MPUs of the range in them")
    assert sv.valid == 1
    if name in ("C2", "C2_ragged"):
        assert bricks == 1000 and dead >= 500 and dead < bricks  # the CPU model of cull_one gives 625
    if name == "C1":
        assert bricks == 27 and abs(dead - 1) <= 1 and bricks - dead >= 1  # 1, give or take the rounding
    if name == "C3_64":
        assert 0 < dead < bricks
    assert np.count_nonzero(passed) > 0


@pytest.mark.parametrize("seed", range(40))
def test_fuzz_trees_dead_bricks(oracle, seed):
    """Every primitive and op type, warps, matrices, at 32^3 cells: a tree the rule does not
    cover has no dead brick at all; one it covers has none with an S1 survivor."""
    model = fuzz_tree(seed)
    sv, _, _ = check_dead_bricks(oracle, f"fuzz{seed}", model, 4.0 / 32)
    if not sv.valid:
        assert not sv.dead.any() and not sv.root_zero.any()


def test_fuzz_trees_cover_both_outcomes():
    got = [Sieve(fuzz_tree(s), 4.0 / 32, f"cover{s}") for s in range(12)]
    assert any(s.valid and s.dead.any() for s in got) and any(not s.valid for s in got)


def test_disc_and_ricci_trees_have_no_dead_brick():
    for tag, model in (("disc", disc_tree()), ("ricci", ricci_tree())):
        sv = Sieve(model, 4.0 / 32, tag)
        assert sv.agree == 1 and sv.valid == 0 and not sv.dead.any(), tag


def test_tree_without_ops_needs_every_primitive():
    model = synth.make_config("C1")[0]
    sv = Sieve(model, synth.make_config("C1")[1], "c1set")
    assert sv.valid == 1 and int(sv.root_zero[0]) == 1 and int(sv.root_zero[1]) == 0
    m2, cs, _ = synth.make_config("C2")
    sv2 = Sieve(m2, cs, "c2set")
    assert int(sv2.root_zero[0]) == 0xff and int(sv2.root_zero[1]) == 0


def test_far_tree_every_brick_dead():
    model = far_tree()
    sv = Sieve(model, synth.make_config("C2")[1], "far")
    assert sv.valid == 1 and sv.dead.all()
    assert soa.mpu_dims(synth.make_config("C2")[1], *model.bbox)[0] == 19
