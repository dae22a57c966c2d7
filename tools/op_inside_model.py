"""Op-box pruning tests a wave's box proves useless (CPU model; DESIGN.md §4, op-inside masks).

Every op deeper than 3 carries the reference's op-box pruning test; it cannot prune when the
wave's whole box lies inside the op's box along one axis (op_inside_box, psgpu_model.h).  For the
MPUs of an oracle run this counts, per walk, the deep ops that are live (their subtree is not
wholly culled: batch_live.mpu_masks) and the share of them whose bit the predicate sets
("all-in"), with the all-out (no S2 corner inside along any axis) and mixed shares for the MPU
boxes:

    per surface MPU / per S1 survivor   one k_mpu walk, the MPU's own masks
    per 64-record vertex batch          k_vertex / k_finish: the AND over the batch's MPUs
                                        (groups-of-4 queue model, batch_live.simulate)
    per S1 brick                        the 2x2x2 brick's box (S1 keeps zero masks; what it leaves)

    python tools/op_inside_model.py [C3] [C5]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, d) for d in ("oracle", "tools", "")]
import batch_live  # noqa: E402
from parsip_amd import soa, synth  # noqa: E402

F = np.float32


def op_tree(model):
    """Per op: depth and the primitives of its subtree."""
    n = model.ct_ops
    depth, prims = np.zeros(n, np.int64), [None] * n
    O = model.ops

    def rec(op, d):
        depth[op] = d
        kind, L, R = int(O["opChildKind"][0, op]), int(O["opLeftChild"][0, op]), int(O["opRightChild"][0, op])
        ps = []
        ps += rec(L, d + 1) if kind & 2 else [L]
        ps += rec(R, d + 1) if kind & 1 else [R]
        prims[op] = ps
        return ps

    if n:
        rec(0, 0)
    return depth, prims


def op_boxes(model):
    n = model.ct_ops
    lo = np.stack([model.ops[f"vBoxLo{c}"][0, :n] for c in "XYZ"], 1).astype(F)
    hi = np.stack([model.ops[f"vBoxHi{c}"][0, :n] for c in "XYZ"], 1).astype(F)
    return lo, hi


def inside_bits(o, ext, lo, hi):
    """op_inside_box in fp32 for boxes [o, o + ext] (ext = 7 cs for an MPU): (boxes, ops) bool."""
    with np.errstate(invalid="ignore", over="ignore"):
        top = (o + F(ext)).astype(F)
        mag = np.maximum(np.abs(o), np.abs(top))
        m = (F(0.002) + F(1e-5) * mag).astype(F)
        ok = mag < F(1e30)
        g0, g1 = (o - m).astype(F)[:, None, :], (top + m).astype(F)[:, None, :]
        return ((lo[None] <= g0) & (g1 <= hi[None]) & ok[:, None, :]).any(2)


def corner_classes(o, cs, lo, hi):
    """all-in / all-out over the 512 S2 corners of each MPU, by the reference's per-point test."""
    cc = (o[:, :, None] + (np.arange(8, dtype=F) * F(cs)).astype(F)[None, None, :]).astype(F)
    per = (cc[:, None] >= lo[None, :, :, None]) & (hi[None, :, :, None] >= cc[:, None])
    return per.all(3).any(2), ~per.any(3).any(2)


def live_ops(culled, prims, deep):
    """(walks, ops): deep op whose subtree is not wholly culled."""
    out = np.zeros((len(culled), len(prims)), bool)
    for k in np.flatnonzero(deep):
        out[:, k] = ~culled[:, prims[k]].all(1)
    return out


def report(label, live, inside, extra=""):
    n = max(len(live), 1)
    tot = int(live.sum())
    print(f"{label:42s} {tot / n:6.2f} live deep ops per walk, all-in {100.0 * (live & inside).sum() / max(tot, 1):5.1f} %{extra}")


def main(argv):
    import psoracle

    for name in [a for a in argv if not a.startswith("-")] or ["C3"]:
        model, cs, _ = synth.make_config(name)
        om = psoracle.polygonize(model, cs, threads=8)
        passed, V = om.stats[:, 0] > 0, om.stats[:, 2].astype(np.int64)
        dims = soa.mpu_dims(cs, *model.bbox)
        depth, prims = op_tree(model)
        deep = depth > 3
        lo, hi = op_boxes(model)
        org = soa.mpu_origins(cs, *model.bbox)
        culled = batch_live.mpu_masks(model, cs)
        live = live_ops(culled, prims, deep)
        ins = inside_bits(org, F(7.0) * F(cs), lo, hi)
        print(f"{name}: {len(org)} MPUs, {int(passed.sum())} pass S1, {int((V > 0).sum())} with a surface; "
              f"{int(deep.sum())} of {model.ct_ops} ops deeper than 3")
        surf = V > 0
        all_in, all_out = corner_classes(org[surf], cs, lo, hi)
        ls = live[surf]
        t = max(int(ls.sum()), 1)
        report("surface MPUs (k_mpu)", ls, ins[surf],
               f"; S2 corners: all-in {100.0 * (ls & all_in).sum() / t:.1f} %, all-out {100.0 * (ls & all_out).sum() / t:.1f} %, "
               f"mixed {100.0 * (ls & ~all_in & ~all_out).sum() / t:.1f} %")
        report("S1 survivors (k_mpu, with field bounds off)", live[passed], ins[passed])
        # vertex batches: 64 consecutive records of a shard; the walk's masks are the AND over its MPUs
        order = batch_live.s1_queue_order(dims, passed)  # blocks of 4 queued S1 survivors reserve together
        bl, bi = [], []
        for w in batch_live.simulate(V, order, 4):
            for b in range(0, len(w), 64):
                ws = np.unique(w[b:b + 64])
                bl.append(live_ops(culled[ws].all(0)[None], prims, deep)[0])
                bi.append(ins[ws].all(0))
        report("64-record vertex batches (groups of 4)", np.array(bl), np.array(bi))
        # S1 bricks: the box of 2x2x2 MPUs (15 cells: the far corners of the far MPUs)
        i, j, k = np.meshgrid(*[np.arange(0, d, 2) for d in dims], indexing="ij")
        first = ((i * dims[1] + j) * dims[2] + k).reshape(-1)
        bo = org[first]
        # culling over the brick box: batch_live's formula on a box of 14 cs + the MPUs' 7 cs
        saved = batch_live.soa.mpu_origins
        try:
            batch_live.soa.mpu_origins = lambda *a, **kw: bo
            bc = batch_live.mpu_masks(model, 2.0 * cs)  # eg = 7 (2 cs) + 0.001: the brick's extent
        finally:
            batch_live.soa.mpu_origins = saved
        report("S1 bricks (k_precheck keeps zero masks)", live_ops(bc, prims, deep), inside_bits(bo, F(14.0) * F(cs), lo, hi))


if __name__ == "__main__":
    main(sys.argv[1:])
