"""Live primitives per 64-record vertex batch (CPU model; DESIGN.md §4, block reservation).

A k_vertex / k_finish wave takes 64 consecutive records of one vertex shard queue and walks every
primitive that is live for any of the MPUs those records belong to (cull_mask_mpus: the AND of
the MPUs' culling masks).  This computes the per-MPU masks on the CPU with cull_one's sphere form
(psgpu_model.h; the kernels' box form culls a few per cent more: tools/cull_pairs.py) on the MPU box grown by 7 cs + 0.001, as k_precheck makes them, takes a queue
layout -- simulated, or downloaded from the GPU with Polygonizer.vertex_queue() -- and reports
the vertex-weighted mean and histogram of live primitives per batch.

    python tools/batch_live.py [C3]          # CPU only: per MPU, random neighbours, groups of G
    python tools/batch_live.py C3 --gpu      # the queue of a run on device 0 as well
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, d) for d in ("oracle", "")]
from parsip_amd import soa, synth  # noqa: E402
from parsip_amd.soa import NodeType  # noqa: E402

BUCKETS = ("[0,4)", "[4,8)", "[8,12)", "[12,16)", ">=16")
F = np.float32


def cull_segments(model):
    """CullSeg of every primitive, as psgpu_set_model makes them (psgpu_host.cpp): a, u, invUU,
    radius, tmin, tmax, axisClear; radius +inf = never culled."""
    P = model.prims
    n = int(P["ctPrims"][0])
    a = np.stack([P[f"pos{c}"][0, :n] for c in "XYZ"], 1).astype(F)
    d = np.stack([P[f"dir{c}"][0, :n] for c in "XYZ"], 1).astype(F)
    r0, r1 = P["resX"][0, :n].astype(F), P["resY"][0, :n].astype(F)
    typ = P["skeletType"][0, :n].astype(np.int64)
    ok = (P["idxMatrix"][0, :n] == 0) & np.isfinite(a).all(1)
    u = np.zeros((n, 3), F)
    radius = np.full(n, np.inf, F)
    tmin, tmax, clear = np.zeros(n, F), np.ones(n, F), np.full(n, -np.inf, F)
    for i in range(n):
        t = typ[i]
        c = bool(ok[i])
        if t == NodeType.LINE:
            ud = d[i].astype(np.float64) - a[i]
            c = c and np.isfinite(d[i]).all() and float(ud @ ud) > 1e-6
        elif t == NodeType.CUBE:
            c = c and np.isfinite(r0[i]) and r0[i] >= 0
        elif t == NodeType.CYLINDER:
            n2 = float(d[i].astype(np.float64) @ d[i].astype(np.float64))
            c = (c and np.isfinite(d[i]).all() and abs(n2 - 1.0) < 1e-4 and r0[i] >= 0 and r1[i] >= 0
                 and np.isfinite(r0[i]) and np.isfinite(r1[i]))
        elif t != NodeType.POINT:
            c = False
        if not c:
            if t == NodeType.TRIANGLE:
                radius[i] = -np.inf  # field exactly 0 everywhere
            continue
        radius[i] = 0.0
        if t == NodeType.LINE:
            u[i] = d[i] - a[i]
            tmin[i], tmax[i] = -np.inf, np.inf
        elif t == NodeType.CYLINDER:
            u[i] = r1[i] * d[i]
            radius[i] = r0[i]
            clear[i] = 0.05
            if not (u[i].astype(np.float64) @ u[i].astype(np.float64)) > 0:
                radius[i] = np.inf
        elif t == NodeType.CUBE:
            radius[i] = F(float(r0[i]) * 1.7320508075688772 * (1.0 + 1e-6))
    uu = (u.astype(np.float64) ** 2).sum(1)
    inv = np.where(uu > 0, 1.0 / np.where(uu > 0, uu, 1.0), 0.0).astype(F)
    return dict(a=a, u=u, invUU=inv, radius=radius, tmin=tmin, tmax=tmax, clear=clear)


def mpu_masks(model, cs, begin=0, end=None):
    """culled[w, i]: primitive i is exactly +0 over MPU slot w's grown box (cull_mask_from with
    cull_one, fp32 as the device evaluates them)."""
    S = cull_segments(model)
    o = soa.mpu_origins(cs, *model.bbox, begin, end)
    eg = F(F(7.0) * F(cs) + F(0.001))
    x1 = o + eg
    c = (F(0.5) * (o + x1))[:, None, :]
    hv = F(0.5) * (x1 - o)
    h = (np.sqrt((hv * hv).sum(1, dtype=F)) * F(1.0001) + F(1e-6))[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        dv = c - S["a"][None]
        t = ((dv * S["u"][None]).sum(2, dtype=F) * S["invUU"][None])[:, :, None]
        lv = dv - t * S["u"][None]
        line = np.sqrt((lv * lv).sum(2, dtype=F))
        tc = np.minimum(np.maximum(t[:, :, 0], S["tmin"][None]), S["tmax"][None])[:, :, None]
        ev = dv - tc * S["u"][None]
        d = (np.sqrt((ev * ev).sum(2, dtype=F)) - S["radius"][None]) - h
        return (d > 0) & (d * d >= F(1.02)) & (line - h > S["clear"][None])


def batch_live(culled, shards, per=64):
    """Vertex-weighted mean and histogram (vertex shares in %, BUCKETS) of live primitives per
    batch of `per` consecutive records; shards: per shard, the records' MPU slots in queue order."""
    n = culled.shape[1]
    live, wts = [], []
    for w in shards:
        w = np.asarray(w, np.int64)
        for b in range(0, len(w), per):
            ws = np.unique(w[b:b + per])
            live.append(n - int(culled[ws].all(0).sum()))
            wts.append(min(per, len(w) - b))
    live, wts = np.asarray(live), np.asarray(wts, np.float64)
    hist = np.zeros(len(BUCKETS))
    np.add.at(hist, np.minimum(live // 4, len(BUCKETS) - 1), wts)
    return float((live * wts).sum() / wts.sum()), 100.0 * hist / wts.sum()


def per_mpu_live(culled, V):
    """The floor: every batch within one MPU (k_mpu's own row: one MPU per wave)."""
    sel = np.flatnonzero(V)
    return batch_live(culled, [np.repeat(s, V[s]) for s in sel], per=1 << 30)


def s1_queue_order(dims, queued):
    """MPU slots in the order k_precheck queues them: 2x2x2 bricks in raster order, a brick's
    survivors (MPU g = bx*4 + by*2 + bz) as consecutive entries."""
    idx = np.flatnonzero(queued)
    i, j, k = idx // (dims[1] * dims[2]), (idx // dims[2]) % dims[1], idx % dims[2]
    nb = [(d + 1) // 2 for d in dims]
    brick = ((i // 2) * nb[1] + j // 2) * nb[2] + k // 2
    g = (i & 1) * 4 + (j & 1) * 2 + (k & 1)
    return idx[np.lexsort((g, brick))]


def simulate(V, order, group, seed=0, nshards=64):
    """Shard queues when groups of `group` queue-consecutive MPUs reserve together and the groups
    reach the shards in an unrelated order (group 1: today's random neighbours)."""
    rng = np.random.default_rng(seed)
    groups = [order[g:g + group] for g in range(0, len(order), group)]
    shards = [[] for _ in range(nshards)]
    for n, gi in enumerate(rng.permutation(len(groups))):
        for s in groups[gi]:
            if V[s]:
                shards[n % nshards].append(np.repeat(s, V[s]))
    return [np.concatenate(s) if s else np.zeros(0, np.int64) for s in shards]


def from_queue(queue):
    """Shard queues from Polygonizer.vertex_queue()."""
    return [recs[:, 0].astype(np.int64) for recs in queue[1]]


def fmt(name, res):
    mean, hist = res
    return f"{name:34s} " + " ".join(f"{h:5.1f}" for h in hist) + f"   mean {mean:.2f}"


def main(argv):
    import psoracle

    name = next((a for a in argv if not a.startswith("-")), "C3")
    model, cs, _ = synth.make_config(name)
    om = psoracle.polygonize(model, cs, threads=8)
    V = om.stats[:, 2].astype(np.int64)
    dims = soa.mpu_dims(cs, *model.bbox)
    culled = mpu_masks(model, cs)
    order = s1_queue_order(dims, om.stats[:, 0] > 0)
    print(f"{name}: {len(V)} MPUs, {len(order)} queued, {int((V > 0).sum())} with vertices, V = {int(V.sum())}")
    print(f"{'vertex share by live primitives':34s} " + " ".join(f"{b:>5s}" for b in BUCKETS))
    print(fmt("per MPU (floor)", per_mpu_live(culled, V)))
    print(fmt("random neighbours", batch_live(culled, simulate(V, order, 1))))
    # the S2 queue holds the S1 survivors k_precheck's field bounds could not prove empty: between
    # every survivor (more surface-less MPUs in a group) and the MPUs with vertices alone
    surf = s1_queue_order(dims, V > 0)
    for g in (2, 4, 8):
        print(fmt(f"groups of {g}, every S1 survivor", batch_live(culled, simulate(V, order, g))))
        print(fmt(f"groups of {g}, surface MPUs only", batch_live(culled, simulate(V, surf, g))))
    print(fmt("whole queue in S1 order", batch_live(culled, [np.repeat(order, V[order])])))
    if "--gpu" in argv:
        from parsip_amd import gpu

        poly = gpu.Polygonizer(0)
        poly.set_model(model)
        poly.run(cs)
        print(fmt("GPU queue (vertex_queue)", batch_live(culled, from_queue(poly.vertex_queue()))))
        poly.close()


if __name__ == "__main__":
    main(sys.argv[1:])
