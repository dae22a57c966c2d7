"""The box bounds of the culling masks and of the S1 field proofs on the CPU (psgpu_model.h:
cull_one with the box's half-extents, prim_interval), through tests/cpp/cullbound_check.cpp
(cullbound_util.py).

Boxes and primitives: whenever the predicate culls a primitive over a box, the reference's fp32
dist2 is >= 1 at the box's corners, centre, face centres, the box point nearest the primitive
and 64 random points; whatever the sphere form culls the box form culls; and the reference's
field at those points lies in the primitive's interval, which is never wider than the sphere
form's.  Models: no MPU the oracle gives vertices is called +0 by the masks or proven empty by
the host model of the bounds, and C3's live-pair counts at 64^3 cells are the recorded ones."""
import json

import numpy as np
import pytest

import cullbound_util as U
from sieve_util import fuzz_tree

# name -> (seed, scale, offset, sanitized build): unit scale at the origin (under AddressSanitizer
# and UBSan), far from the origin (where a box's centre rounds), and a small scene
SOUPS = {"unit_sanitized": (1, 1.0, (0.0, 0.0, 0.0), True),
         "offset": (2, 1.0, (1000.0, -500.0, 250.0), False),
         "small": (3, 0.3, (0.0, 0.0, 0.0), False)}


@pytest.mark.parametrize("name", list(SOUPS))
def test_box_forms_are_sound_and_cull_no_less(name):
    seed, scale, offset, sanitize = SOUPS[name]
    model = U.prim_soup(seed, scale, offset)
    boxes = U.adversarial_boxes(model, seed, scale)
    c = U.Check(model, f"soup_{name}", boxes=boxes, seed=seed, sanitize=sanitize)
    print(f"{name}: {len(boxes)} boxes x 128 primitives: culled {c.culled_sphere} -> {c.culled_box}; "
          f"{c.intervals_tested} intervals; {c.stderr.strip()}")
    assert c.pairs_tested == 128 * len(boxes) and c.intervals_tested > c.pairs_tested // 2
    assert c.culled_sphere > c.pairs_tested // 10 and c.culled_box > c.culled_sphere  # both outcomes, and a gain
    assert c.unsound_culls == 0, c.stderr
    assert c.lost_culls == 0, c.stderr
    assert c.unsound_intervals == 0, c.stderr
    assert c.wider_intervals == 0, c.stderr


def check_model(oracle, tag, model, cs):
    c = U.Check(model, tag, cs=cs)
    om = oracle.polygonize(model, cs, threads=8, keep=False)
    assert len(om.stats) == len(c.zero_box)
    has = om.stats[:, 2] != 0
    for what, flags in (("+0 by the masks", c.zero_box), ("proven empty", c.proven_box), ("+0 (sphere)", c.zero_sphere),
                        ("proven empty (sphere)", c.proven_sphere)):
        bad = np.flatnonzero(flags & has)
        assert len(bad) == 0, f"{tag}: {len(bad)} MPUs with vertices are called {what}, first {int(bad[0])}"
    # the box form gives up nothing the sphere form had
    assert not (c.zero_sphere & ~c.zero_box).any() and not (c.proven_sphere & ~c.proven_box).any()
    return c, has


@pytest.mark.parametrize("name", ["C1", "C2", "C3"])
def test_configs_at_64_cells(oracle, name):
    model, cs = U.coarse(name, 64)
    c, has = check_model(oracle, name, model, cs)
    assert has.any() and c.proven_box.any() and c.zero_box.any()
    if name == "C3":
        with open(U.GOLDEN) as f:
            want = json.load(f)["cpu_C3_64"]
        assert c.counts() == want
        live = c.live
        assert (live[:, 1] <= live[:, 0]).all() and live[0, 1, 0] < live[0, 0, 0] and live[1, 1, 0] < live[1, 0, 0]


@pytest.mark.parametrize("seed", range(40))
def test_fuzz_trees_at_32_cells(oracle, seed):
    check_model(oracle, f"fuzz{seed}", fuzz_tree(seed), 4.0 / 32)


def test_fuzz_trees_cover_both_verdicts():
    got = [U.Check(fuzz_tree(s), f"cover{s}", cs=4.0 / 32) for s in range(2, 40, 3)]  # the cullable third
    assert any(c.zero_box.any() for c in got) and any(c.proven_box.any() for c in got)
