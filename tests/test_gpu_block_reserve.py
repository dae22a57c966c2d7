"""k_mpu's block-level reservation of the vertex record queue (mpu_body, psgpu_device.h):
the mesh stays the oracle's bit for bit whatever a block holds (partial blocks, MPUs without a
surface among MPUs with one, shards that overflow), the queue stays dense and contiguous per MPU,
a block's MPUs lie back to back in one shard, and the 64-record batches of the vertex walks then
see fewer live primitives (tools/batch_live.py on the queue the GPU wrote)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from parsip_amd import gpu, synth
from parity_util import assert_mesh_matches

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import batch_live  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
STAMP_WAVES = 1 << 18  # k_mpu waves recorded: more than any grid of C2 / C3

# Live primitives per 64-record batch (vertex-weighted mean, tools/batch_live.py) of the C3 queue
# the earlier per-MPU reservation wrote (one reservation per MPU into shard d & 63, the kernels
# otherwise the same; commit 3e38f9d is the last tree that compiles that variant), measured on
# an MI355X, 2026-10-19 (k_front's queue order keeps some neighbours together: the CPU model
# gives 6.46 for unrelated neighbours) and the model's value for one reservation per block.
PARENT_C3_MEAN_LIVE = 6.01
MODEL_BLOCK_MEAN_LIVE = 4.80


@pytest.fixture(scope="module")
def c2(oracle):
    model, cs, _ = synth.make_config("C2")
    return model, cs, oracle.polygonize(model, cs, threads=8)


@pytest.fixture(scope="module")
def c3(oracle):
    model, cs, _ = synth.make_config("C3")
    return model, cs, oracle.polygonize(model, cs, threads=8)


@pytest.fixture(scope="module")
def c2_ranges(oracle, c2):
    """MPU ranges of C2 that queue exactly n S2 MPUs (S1 survivors; the field-bound proofs are
    off in the test), n = 1, 2, 3, 5, with their oracle meshes; for n > 1 the range mixes MPUs
    with a surface and S1 survivors without one."""
    model, cs, om = c2
    passed, V = om.stats[:, 0] > 0, om.stats[:, 2]
    idx = np.flatnonzero(passed)
    out = {}
    for n in (1, 2, 3, 5):
        for a in range(len(idx) - n + 1):
            surf = V[idx[a:a + n]] > 0
            if surf.any() and (n == 1 or not surf.all()):
                b, e = int(idx[a]), int(idx[a + n - 1]) + 1
                assert int(passed[b:e].sum()) == n
                out[n] = (b, e, oracle.polygonize(model, cs, b, e, threads=2))
                break
    assert sorted(out) == [1, 2, 3, 5]
    return out


@pytest.mark.parametrize("jit,front,split", [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1)])
def test_partial_and_mixed_blocks(gpu_poly, c2, c2_ranges, jit, front, split):
    """Blocks with 1, 2 and 3 MPUs, a full block followed by a block of one, and blocks whose
    MPUs partly have no surface (they reserve 0 records), through k_mpu and k_front, one and two
    waves per MPU, interpreter and generated kernels (k_front and the split are generated only)."""
    model, cs, _ = c2
    try:
        gpu_poly.set_option(gpu.OPT_JIT, jit)
        gpu_poly.set_option(gpu.OPT_BOUND, 0)  # every S1 survivor is queued: the oracle's count
        gpu_poly.set_option(gpu.OPT_TREE_SPLIT, split)
        gpu_poly.set_model(model)
        gpu_poly.jit_wait()
        assert gpu_poly.jit_active == bool(jit)
        gpu_poly.set_option(gpu.OPT_FRONT, front)
        for n, (b, e, om) in c2_ranges.items():
            info = gpu_poly.run(cs, b, e)
            assert info.ctFieldMPUs == n
            assert bool(info.launchFlags & gpu.LAUNCH_FRONT) == bool(front), (n, info.launchFlags)
            assert bool(info.launchFlags & gpu.LAUNCH_TREE_SPLIT) == bool(split), (n, info.launchFlags)
            assert_mesh_matches(gpu_poly.download(), gpu_poly.stats(), om)
    finally:
        gpu_poly.set_option(gpu.OPT_JIT, 1)
        gpu_poly.set_option(gpu.OPT_BOUND, 1)
        gpu_poly.set_option(gpu.OPT_TREE_SPLIT, 0)
        gpu_poly.set_option(gpu.OPT_FRONT, 2)


def test_grow_and_rerun(c2):
    """A fresh context whose vertex shards hold half their mean share of C2's records: the first
    run overflows them (within a block too: its later MPUs fall past the shard's end while the
    first fits), finish() grows the queues, re-runs and returns the exact mesh."""
    model, cs, om = c2
    V = int(om.stats[:, 2].sum())
    assert V // 2 >= 64
    poly = gpu.Polygonizer(0)
    try:
        poly.set_option(gpu.OPT_CAPACITY, V // 2)  # 64 shards of V / 128 records; the mean share is V / 64
        poly.set_model(model)
        info = poly.run(cs)
        assert info.launchFlags & gpu.LAUNCH_RERUN
        assert info.ctVertices == V
        assert_mesh_matches(poly.download(), poly.stats(), om)
    finally:
        poly.close()


def mpu_blocks(poly) -> np.ndarray:
    """(blocks, 4): the MPU each wave of each k_mpu block of the last run worked on (NONE: none),
    from the per-wave timeline (OPT_STAMPS), whose k_mpu records are indexed block * 4 + wave."""
    L, cap = gpu.load(), ctypes.c_uint32()
    gpu._check(L.psgpu_download_stamps(poly._ctx, None, ctypes.byref(cap)), "psgpu_download_stamps")
    n = cap.value
    assert n == STAMP_WAVES
    raw = np.zeros(len(gpu.STAMP_KERNELS) * n * 3 + n * 8, np.uint64)
    gpu._check(L.psgpu_download_stamps(poly._ctx, raw.ctypes.data, ctypes.byref(cap)), "psgpu_download_stamps")
    rec = raw[:len(gpu.STAMP_KERNELS) * n * 3].reshape(len(gpu.STAMP_KERNELS), n, 3)[1]
    item = (rec[:, 2] & np.uint64(NONE)).astype(np.int64)
    item[rec[:, 0] == 0] = NONE
    return item.reshape(-1, 4)


def run_with_queue(poly, model, cs, split=0):
    try:
        poly.set_option(gpu.OPT_TREE_SPLIT, split)
        poly.set_model(model)
        poly.jit_wait()
        poly.set_option(gpu.OPT_STAMPS, STAMP_WAVES)
        info = poly.run(cs)
        assert bool(info.launchFlags & gpu.LAUNCH_TREE_SPLIT) == bool(split)
        counts, shards = poly.vertex_queue()
        return info, counts, shards, mpu_blocks(poly)
    finally:
        poly.set_option(gpu.OPT_STAMPS, 0)
        poly.set_option(gpu.OPT_TREE_SPLIT, 0)


@pytest.fixture(scope="module")
def c3_queue(gpu_poly, c3):
    model, cs, _ = c3
    return run_with_queue(gpu_poly, model, cs)


def check_queue(info, counts, shards, blocks, om, mpb):
    V = om.stats[:, 2].astype(np.int64)
    assert int(counts.sum()) == int(V.sum()) == info.ctVertices
    where = {}  # MPU -> (shard, first record)
    for s, recs in enumerate(shards):
        assert len(recs) == counts[s]
        w, vid = recs[:, 0].astype(np.int64), recs[:, 1].astype(np.int64)
        starts = np.flatnonzero(np.r_[True, w[1:] != w[:-1]]) if len(w) else np.zeros(0, np.int64)
        lens = np.diff(np.r_[starts, len(w)])
        # every run of one MPU is the whole MPU, in vid order
        np.testing.assert_array_equal(lens, V[w[starts]], err_msg=f"shard {s}: an MPU's records are split")
        np.testing.assert_array_equal(vid, np.arange(len(w)) - np.repeat(starts, lens), err_msg=f"shard {s}: vid order")
        for m, a in zip(w[starts], starts):
            assert m not in where, f"MPU {m} in two places"
            where[int(m)] = (s, int(a))
    assert sorted(where) == list(np.flatnonzero(V))
    grouped = 0
    for blk, row in enumerate(blocks):
        mpus = list(dict.fromkeys(int(m) for m in row if m != NONE))  # slot order; two waves per MPU with the split
        assert len(mpus) <= mpb
        mpus = [m for m in mpus if V[m] > 0]
        for m in mpus:
            assert where[m][0] == blk % 64, (blk, m, where[m])
        for m0, m1 in zip(mpus, mpus[1:]):  # one reservation: the block's MPUs back to back, in slot order
            assert where[m1][1] == where[m0][1] + V[m0], (blk, mpus)
        grouped += len(mpus)
    assert grouped == len(where)  # every MPU with records was some block's


@pytest.mark.parametrize("split", [0, 1])
def test_queue_invariants_c2(gpu_poly, c2, split):
    model, cs, om = c2
    check_queue(*run_with_queue(gpu_poly, model, cs, split), om, 2 if split else 4)


def test_queue_invariants_c3(c3, c3_queue):
    check_queue(*c3_queue, c3[2], 4)


def test_batches_are_coherent(c3, c3_queue):
    """The vertex-weighted mean of live primitives per 64-record batch of C3's queue, by the CPU
    model on the queue the GPU wrote, is below the midpoint of the parent's measured value and the
    model's value for one reservation per block (room for arrival-order effects the model does not
    have; a grouping that silently stops working lands at the parent's value)."""
    model, cs, _ = c3
    mean, hist = batch_live.batch_live(batch_live.mpu_masks(model, cs), batch_live.from_queue(c3_queue[1:3]))
    print("C3 live primitives per batch:", " ".join(f"{h:.1f}" for h in hist), f"mean {mean:.2f}")
    assert mean < 0.5 * (PARENT_C3_MEAN_LIVE + MODEL_BLOCK_MEAN_LIVE)
