"""The op-inside mask predicate (op_inside_box, psgpu_model.h) on the CPU: for every MPU and every
op whose bit the predicate sets, the reference's own per-point op-box test holds at every point a
walk evaluates under that MPU -- the 512 S2 corners, and for every oracle vertex its four edge
samples, its root and its three normal points -- so skipping the test there changes nothing.
The predicate is the code under test (compiled from the header by tests/cpp/op_inside_check.cpp);
the test `in`, the lattice and the vertices come from the oracle side (op_inside_util.ref_in,
soa.mpu_origins, psoracle)."""
import numpy as np
import pytest

from parsip_amd import soa
import op_inside_util as U


@pytest.fixture(scope="module")
def oracle_meshes(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            model, cs = U.make_case(name)
            cache[name] = oracle.polygonize(model, cs, threads=8)
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(U.CASES))
def test_set_bits_hold_at_every_walked_point(oracle_meshes, name):
    model, cs = U.make_case(name)
    om = oracle_meshes(name)
    lo, hi = U.op_boxes(model)
    org = soa.mpu_origins(cs, *model.bbox)
    bits = U.mask_bits(U.cpu_masks(name), model.ct_ops)
    assert bits.shape == (len(org), model.ct_ops) and len(org) == len(om.stats)
    depth = U.op_depths(model)
    deep = depth > 3
    assert deep.any() and (depth.max() >= 10 or not name.startswith("chain"))

    # S2 corners: in(q) is an OR over the axes of per-coordinate tests, so it holds at all 512
    # corners exactly when, along some axis, it holds for all 8 coordinates (otherwise the corner
    # made of one failing coordinate per axis fails)
    cc = U.corner_coords(org, cs)                                                     # (M, 3, 8)
    per = (cc[:, None, :, :] >= lo[None, :, :, None]) & (hi[None, :, :, None] >= cc[:, None, :, :])  # (M, K, 3, 8)
    all_in = per.all(3).any(2)
    all_out = ~per.any(3).any(2)
    mixed = ~all_in & ~all_out
    assert not (bits & ~all_in).any(), "a set bit whose op box misses an S2 corner"

    # every oracle vertex: edge samples, root, normal points
    voff = om.vertex_offsets
    checked = 0
    for w in np.flatnonzero(np.diff(voff)):
        k = np.flatnonzero(bits[w])
        if len(k) == 0:
            continue
        pts = U.vertex_points(om.pos[voff[w]:voff[w + 1]], org[w], cs).reshape(-1, 3)
        ok = U.ref_in(pts, lo[k], hi[k])
        assert ok.all(), (name, int(w), k[~ok.all(0)])
        checked += ok.size
    assert checked > 0

    # the inputs exercise every outcome among the deep ops: bits set, all-in, mixed and all-out
    n_set, n_in, n_mixed, n_out = (int(x[:, deep].sum()) for x in (bits, all_in, mixed, all_out))
    print(f"{name}: MPUs {len(org)}, deep ops {int(deep.sum())}: bit set {n_set}, all-in {n_in}, mixed {n_mixed}, "
          f"all-out {n_out}; vertex points checked {checked}")
    assert n_set > 0 and n_mixed > 0 and n_out > 0


def test_nan_and_huge_boxes_set_no_bit():
    """NaN compares false and a lattice beyond 1e30 sets nothing (op_inside_axis's guard)."""
    import os
    import subprocess

    exe = U.check_exe()
    d = os.path.dirname(exe)
    F = np.float32
    ops = np.array([[-1, -1, -1, 1, 1, 1], [np.nan, -1, -1, 1, np.nan, 1], [-np.inf, -np.inf, -np.inf, np.inf, np.inf, np.inf],
                    [-1, np.nan, np.nan, np.nan, np.nan, np.nan]], F)
    org = np.array([[0, 0, 0], [np.nan, 5, 5], [1e31, 1e31, 1e31], [0.95, 0.95, 0.95], [5, 5, 0]], F)
    with open(os.path.join(d, "edge.in"), "wb") as f:
        f.write(np.array([len(ops), len(org)], np.uint32).tobytes() + F(0.01).tobytes() + np.uint32(0).tobytes())
        f.write(ops.tobytes() + org.tobytes())
    subprocess.run([exe, os.path.join(d, "edge.in"), os.path.join(d, "edge.out")], check=True, timeout=60)
    bits = U.mask_bits(np.fromfile(os.path.join(d, "edge.out"), np.uint64).reshape(-1, 2), len(ops))
    want = np.array([[1, 1, 1, 0],   # inside op 0 on every axis, op 1 along z only, the infinite box
                     [0, 0, 1, 0],   # a NaN x origin: y and z still decide (outside the unit boxes)
                     [0, 0, 0, 0],   # magnitude >= 1e30: no bit, not even the infinite box's
                     [0, 0, 1, 0],   # 0.95 + 0.07 = 1.02 > 1: straddles the unit boxes
                     [1, 1, 1, 0]], bool)  # outside along x and y, inside along z
    np.testing.assert_array_equal(bits, want)
