"""S2 walks only the octants S1's field bounds left undecided (DESIGN.md §4 "S2 octants"), on the
CPU: the plan (which lane walks which octant in which pass, and how the walked bits and the
decided octants' constants make the canonical inside bits) checked by the host program's own
exhaustive run, and the soundness of what S2 no longer evaluates: for every queued MPU and every
octant the host model of S1's bounds decides, the oracle's field at the octant's 64 lattice points
-- built with the device's fp32 expressions, in the reference's SIMD groups -- lies on the decided
side of 0.5."""
import json

import numpy as np
import pytest

import s2_octants_util as S
from parsip_amd import synth

_VERDICTS = {}


def verdicts(oracle, name):
    if name not in _VERDICTS:
        model, cs = S.make_case(name)
        om = oracle.polygonize(model, cs, threads=8, keep=False)
        _VERDICTS[name] = S.Verdicts(model, cs, om.stats[:, 0], name)
    return _VERDICTS[name]


def test_plan_and_assembly():
    """All 256 masks: every undecided octant walked exactly once and in order, fillers repeat an
    octant of their own pass, ceil(U / 4) passes; random 512-bit patterns rebuilt exactly."""
    rc, err = S.plan_check()
    assert rc == 0, err


def test_plan_and_assembly_sanitized():
    rc, err = S.plan_check(sanitize=True)
    assert rc == 0, err


@pytest.mark.parametrize("name", list(S.CASES))
def test_decided_octants_hold_at_every_point(oracle, name):
    v = verdicts(oracle, name)
    assert not np.any(v.outside & v.inside), "an octant proven both outside and inside"
    x, y, z, inside = v.decided_points()
    f = oracle.field_value(v.model, x, y, z)
    wrong = (f >= np.float32(0.5)) != inside
    print(f"{name}: {int(np.count_nonzero(v.queued))} queued, histogram {v.histogram()}, "
          f"{len(f)} decided points, {int(np.count_nonzero(wrong))} on the wrong side")
    assert not wrong.any(), (name, int(np.count_nonzero(wrong)), float(f[wrong][0]))


def test_sanitized_model_agrees(oracle):
    v = verdicts(oracle, "C3_5x3x8")
    model, cs = S.make_case("C3_5x3x8")
    om = oracle.polygonize(model, cs, threads=8, keep=False)
    s = S.Verdicts(model, cs, om.stats[:, 0], "C3_5x3x8_san", sanitize=True)
    np.testing.assert_array_equal(s.queued, v.queued)
    np.testing.assert_array_equal(s.outside, v.outside)
    np.testing.assert_array_equal(s.inside, v.inside)


def test_without_bounds_no_octant_is_decided(oracle):
    model, cs = S.make_case("C2")
    om = oracle.polygonize(model, cs, threads=8, keep=False)
    v = S.Verdicts(model, cs, om.stats[:, 0], "C2_nobound", bound=False)
    np.testing.assert_array_equal(v.queued, om.stats[:, 0] != 0)
    assert not v.outside.any() and not v.inside.any()
    assert set(v.passes[v.queued]) == {2}


@pytest.mark.parametrize("name", ["C2", "C3_64", "C3"])
def test_recorded_histograms(oracle, name):
    """The model's table rows as recorded (C3: the whole config, the row of DESIGN.md §4)."""
    with open(S.GOLDEN) as f:
        want = json.load(f)[name]
    if name == "C3":
        model, cs = synth.make_config("C3")[:2]
        om = oracle.polygonize(model, cs, threads=8, keep=False)
        got = S.Verdicts(model, cs, om.stats[:, 0], "C3").counts()
    else:
        got = verdicts(oracle, name).counts()
    assert got == want


def test_c2_covers_every_plan(oracle):
    """So that the device test cannot pass vacuously: on C2 every count of undecided octants from
    0 to 8 occurs, and some MPU needs two passes."""
    v = verdicts(oracle, "C2")
    hist = v.histogram()
    assert hist == [2, 61, 118, 59, 123, 75, 73, 6, 2]
    assert all(h > 0 for h in hist)
    assert np.count_nonzero(v.passes == 2) > 0
    assert np.count_nonzero(v.passes[v.queued] == 0) == hist[0]


def test_front_and_mpu_kernels_keep_their_registers():
    """The run-time loop round the S2 walk must not leave the walk's uniform work live across it
    (profiles/s2_octants_kernel_resources.txt): on C3's structure tier k_mpu and k_front keep no
    SGPR in VGPR lanes, the tree-split k_front at most the 20 it was measured with, nothing has
    scratch, and no kernel is below the waves per SIMD it was measured at.  (A define of its own
    in the flags: a compile no other test of the process has made, so its code object is written.)"""
    import os
    import sys

    sys.path.insert(0, os.path.join(S.ROOT, "tools"))
    import kernel_resources as kr

    ks = kr.compile_variant("C3", 1 | 4, {"PSGPU_JIT_FLAGS": "-DPSGPU_S2_OCTANTS_RESOURCES=1"})
    for name, (waves, spill) in {"jit_mpu": (7, 0), "jit_front": (6, 0), "jit_front_s": (6, 20),
                                 "jit_precheck": (7, 0), "jit_precheck_s": (7, 0)}.items():
        r = ks[name]
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] <= spill, (name, r)
        assert r["waves_per_simd"] >= waves, (name, r["waves_per_simd"], r["limited_by"], r["vgpr"], r["sgpr"])
