"""Generate tests/golden/reference/: outputs of the compiled reference itself.

Needs the reference library (`make -C oracle ref`, oracle/psref.py); the files it writes are
what lets tests/test_reference.py::test_recorded_* and tests/test_gpu_reference.py run where
the reference is absent.

* ``<name>.npz`` for C1 and the trees of FIXTURE_SEEDS (tests/reference_util.exact_case at
  most 512 MPUs): the raw input SoA bytes (prims, mats, ops), the cell size, the reference's
  per-MPU ctFieldEvals / ctVertices / ctTriangles, MPU-local triangles, positions, normals
  and colours, and FieldComputer::fieldValue at 256 z-consecutive quads plus
  fieldValueAndColor at each quad's first point (all four lanes that point, as the
  polygonizer's vertex stage calls it).  The trees hold no Disc, Ring or RicciBlend, so
  every recorded bit but the normals' is plain IEEE arithmetic and independent of the host
  CPU's rsqrtps / rcpps; normals are compared within 2e-3.
* the same for the trees of BOX_FIXTURES, each in a box whose MPU lattice has three pairwise
  distinct dims (``box<dims>_tree<seed>.npz``; every other fixture's lattice is a cube).
* ``index.json``: the node types in each tree and its sizes.
* ``deviation.json``: the measured distance between the IEEE oracle and the reference on
  trees with Disc / Ring / RicciBlend, and between the two PrepareBBoxes
  (tests/reference_util.measure_deviation / measure_boxes); test_reference.py asserts at
  most twice these.

Usage: python tests/golden/make_reference_goldens.py [--search]
  --search prints a greedy choice of FIXTURE_SEEDS: trees of at most 8 primitives with 200 to
  1,500 vertices that cover every primitive and operator of the family and matrices on and
  off, then cover them again until there are six to eight trees.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import aniso_util as au  # noqa: E402
import psoracle  # noqa: E402
import psref  # noqa: E402
import reference_util as ru  # noqa: E402

from parsip_amd import soa, synth  # noqa: E402

OUT = ru.GOLDEN_REF
FIXTURE_SEEDS = (3, 7, 29, 113, 142, 186, 193, 383)  # what --search printed
MAX_MPUS, MIN_V, MAX_V, N_QUADS = 512, 200, 1500, 256
N_MAX = 8  # small trees: each node weighs on its mesh
# (seed, dims): trees of the same family in boxes that are no cubes (tests/aniso_util.box_for
# around the origin), the three rotations of one shape -- chosen by hand among the seeds below
# 120 for MIN_V to MAX_V vertices and surface MPUs at three or more places along every axis
BOX_FIXTURES = ((43, (8, 5, 3)), (9, (5, 3, 8)), (53, (3, 8, 5)))


def box_case(seed, dims):
    model, cs = ru.exact_case(seed, MAX_MPUS, N_MAX)
    model = au.boxed(model, *au.box_for(dims, (0.0, 0.0, 0.0), cs))
    assert soa.mpu_dims(cs, *model.bbox) == dims
    return model, cs


def wanted():
    return {("p", t) for t in set(ru.EXACT_TYPES)} | {("o", t) for t in ru.EXACT_OPS} | {("m", 0), ("m", 1)}


def covers(model):
    p, o = ru.node_types(model)
    uses_matrix = int(model.prims["idxMatrix"][0, :model.ct_prims].any())
    return {("p", t) for t in p} | {("o", t) for t in o} | {("m", uses_matrix)}


def search(limit=400):
    cand = []
    for s in range(limit):
        model, cs = ru.exact_case(s, MAX_MPUS, N_MAX)
        v = int(psref.polygonize(model, cs).stats[:, 2].sum())
        if MIN_V <= v <= MAX_V:
            cand.append((s, covers(model)))
    need, chosen = wanted(), []
    while need or len(chosen) < 6:
        need = need or wanted()  # covered once with fewer than six trees: cover it again
        s, c = max((sc for sc in cand if sc[0] not in chosen), key=lambda sc: (len(sc[1] & need), -sc[0]))
        assert c & need, f"no candidate covers {need}"
        chosen.append(s)
        need -= c
        if len(chosen) == 8:
            break
    print("FIXTURE_SEEDS =", tuple(sorted(chosen)))


def record(name, model, cs):
    mesh = psref.polygonize(model, cs)
    st = mesh.stats
    assert len(st) <= MAX_MPUS and int(st[:, 2].max()) <= soa.MAX_MPU_VERTEX_COUNT
    assert int(st[:, 3].max()) <= soa.MAX_MPU_TRIANGLE_COUNT
    x, y, z = ru.quads(model, cs, N_QUADS, 12345)
    qf = psref.field_value(model, x, y, z)
    rep = [np.repeat(a[::4], 4) for a in (x, y, z)]
    cf, cc = psref.field_value_and_color(model, *rep)
    np.savez_compressed(
        os.path.join(OUT, name + ".npz"),
        prims=np.frombuffer(model.prims.tobytes(), np.uint8), mats=np.frombuffer(model.mats.tobytes(), np.uint8),
        ops=np.frombuffer(model.ops.tobytes(), np.uint8), cellsize=np.float32(cs),
        evals=st[:, 1].astype(np.uint16), ctv=st[:, 2].astype(np.uint16), ctt=st[:, 3].astype(np.uint16),
        tris=mesh.tris, pos=mesh.pos, nrm=mesh.nrm, col=mesh.col,
        quad_xyz=np.stack([x, y, z], axis=1), quad_field=qf, point_field=cf[::4].copy(), point_colour=cc[::4].copy())
    p, o = ru.node_types(model)
    size = os.path.getsize(os.path.join(OUT, name + ".npz"))
    print(name, len(st), "MPUs", len(mesh.pos), "V", len(mesh.tris), "T", size, "B")
    return {"prims": [ru.TYPE_NAMES[t] for t in p], "ops": [ru.TYPE_NAMES[t] for t in o],
            "ct_prims": model.ct_prims, "ct_ops": model.ct_ops,
            "matrices": bool(model.prims["idxMatrix"][0, :model.ct_prims].any()),
            "mpus": int(len(st)), "vertices": int(len(mesh.pos)), "triangles": int(len(mesh.tris))}


def main():
    assert psref.available(), "the reference library is needed: make -C oracle ref"
    psoracle.build()
    if "--search" in sys.argv:
        return search()
    os.makedirs(OUT, exist_ok=True)
    index = {"generator": "tests/golden/make_reference_goldens.py: PS::SIMDPOLY compiled by `make -C oracle ref` "
                          "(clang++ -O2 -msse4.1 -ffp-contract=off -ftrivial-auto-var-init=zero)",
             "fixtures": {}}
    model, cs, _ = synth.make_config("C1")
    index["fixtures"]["C1"] = record("C1", model, cs)
    for s in FIXTURE_SEEDS:
        model, cs = ru.exact_case(s, MAX_MPUS, N_MAX)
        index["fixtures"][f"tree{s}"] = dict(record(f"tree{s}", model, cs), seed=s)
    for s, dims in BOX_FIXTURES:
        model, cs = box_case(s, dims)
        name = "box" + "x".join(str(d) for d in dims) + f"_tree{s}"
        index["fixtures"][name] = dict(record(name, model, cs), seed=s, dims=list(dims))
    with open(os.path.join(OUT, "index.json"), "w") as f:
        json.dump(index, f, indent=1)
    dev = {"generator": "tests/golden/make_reference_goldens.py (tests/reference_util.measure_deviation, measure_boxes)",
           "note": "IEEE oracle (oracle/psoracle.c, what the HIP path equals bit for bit) against the compiled "
                   "reference; tests/test_reference.py asserts at most 2x these. nrm_max_abs is recorded, not bounded.",
           "approx_trees": ru.measure_deviation(psref, psoracle), "boxes": ru.measure_boxes(psref, psoracle)}
    with open(os.path.join(OUT, "deviation.json"), "w") as f:
        json.dump(dev, f, indent=1)
    print(json.dumps(dev, indent=1))


if __name__ == "__main__":
    main()
