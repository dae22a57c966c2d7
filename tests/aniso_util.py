"""Inputs with non-cubic MPU lattices, shared by tests/test_aniso.py (CPU) and
tests/test_gpu_aniso.py (device): lattices whose three dims are pairwise distinct or contain a 1,
each shape in its three cyclic rotations so that every axis takes every role, ragged MPU ranges
written in terms of dims[1] * dims[2], the fuzz trees in drawn boxes, and the weld's closed
surface in a (6,7,5) box.  synth.make_config and synth.random_model only ever give cubes."""
import numpy as np

import weld_util
from parsip_amd import soa, synth

F = np.float32
CS = 0.0713  # the named lattices' cell size: off the round values

# dims -> centre of the box around C2's tree (content near (0.4, 1.3, 1.3)); the thin lattices
# sit where they cut the surface
FIRST = (0.1, -0.15, 0.05)
LATTICES = {
    (11, 5, 2): (0.39, 1.3, 1.27), (2, 11, 5): FIRST, (5, 2, 11): FIRST,
    (1, 7, 4): (-0.2, 1.42, 1.19), (7, 4, 1): (-0.85, 0.3, 1.16), (4, 1, 7): (0.39, 1.3, 1.27),
    (3, 6, 9): FIRST, (9, 3, 6): FIRST, (6, 9, 3): FIRST,
    (8, 1, 1): (-0.92, -0.33, 0.89), (1, 1, 8): (-1.46, 1.3, -1.24), (1, 8, 1): (-0.3, 0.28, 0.71),
}
WELD_CASE = weld_util.BOXED_NAME


def boxed(model, lo, hi):
    """A copy of the model with the scene box overwritten."""
    m = model.copy()
    m.prims["bboxLo"][0] = np.asarray(lo, F)
    m.prims["bboxHi"][0] = np.asarray(hi, F)
    return m


def box_for(dims, centre, cs):
    """A box whose lattice is exactly ``dims``: 7 * d - 2.5 cells per axis, so the last MPU of
    each axis overhangs the box by 2.5 cells."""
    ext = (7.0 * np.asarray(dims, np.float64) - 2.5) * cs
    lo = (np.asarray(centre, np.float64) - ext / 2).astype(F)
    hi = (lo + ext.astype(F)).astype(F)
    return lo, hi


_C2 = {}


def lattice_case(dims):
    """(C2's tree in the box that gives the lattice ``dims``, cell size).  One tree for all of
    them: the generated kernels compile once."""
    if "model" not in _C2:
        _C2["model"] = synth.make_config("C2")[0]
    model = boxed(_C2["model"], *box_for(dims, LATTICES[dims], CS))
    assert soa.mpu_dims(CS, *model.bbox) == tuple(dims), (dims, soa.mpu_dims(CS, *model.bbox))
    return model, CS


def ranges(dims):
    """name -> MPU range [begin, end) of the lattice."""
    d0, d1, d2 = dims
    nyz = d1 * d2
    n = d0 * nyz
    # begins in an odd x-row (where there is one), mid z-row; ends mid-row several rows on.
    # brick_layout's first / 2 then starts one MPU row before the range.
    b = (nyz if d0 > 1 else 0) + (d1 // 2) * d2 + d2 // 2
    e = n - (d1 // 3 + 1) * d2 + (d2 + 1) // 2
    if e < b + 2:
        e = min(n, b + 2)
    x0 = (d0 // 2) * nyz
    return {"full": (0, n), "ragged": (b, e), "in_row": (x0 + nyz // 3, x0 + nyz // 3 + max(1, nyz // 2)),
            "first": (0, 1), "last": (n - 1, n)}


RANGES = {d: ranges(d) for d in LATTICES}


def fuzz_box_case(seed):
    """test_gpu_fuzz.fuzz_case(seed) in a box drawn from a generator of its own, redrawn until
    the three dims are pairwise distinct; the MPU range redrawn for the new lattice by
    fuzz_case's rule."""
    from test_gpu_fuzz import fuzz_case

    model, cs, _, _, cull, jit, layout = fuzz_case(seed)
    rng = np.random.default_rng(5000 + seed)
    while True:
        lo = rng.uniform(-2.0, -0.6, 3).astype(F)
        hi = rng.uniform(0.6, 2.0, 3).astype(F)
        d = soa.mpu_dims(cs, lo, hi)
        if len(set(d)) == 3:
            break
    total = int(np.prod(d))
    begin = int(rng.integers(0, max(1, total // 3)))
    end = int(rng.integers(max(begin + 1, 2 * total // 3), total + 1))
    return boxed(model, lo, hi), cs, begin, end, cull, jit, layout


def weld_case():
    """(rand3's closed surface in a (6,7,5) box, cell size 0.071, (0, None))."""
    return weld_util.make_case(WELD_CASE)
