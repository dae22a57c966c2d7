// psgpu_plan.h — the launch shape of one polygonization, decided once per enqueue.
//
// One polygonization is two to four launches: k_precheck and k_mpu (or both as k_front), then
// k_vertex and k_finish (or both as k_surface).  plan_launch() picks the kernels, their layouts
// and every grid from a PlanInput and from nothing else: no context, no HIP call, no globals.
// The host (psgpu_host.cpp) fills the input from its context, launches what the plan says, keys
// its hipGraph replay on the plan's bytes and reports it as PsMeshInfo.launchFlags.  LDS sizes
// are not part of it (they need the device header).
//
// The other end of a run is decided here too: judge_run() turns a finished run's counters, its
// plan and the context's capacities into "fits", "grow to these capacities and re-run" or
// "protocol error", and mesh_info() into the PsMeshInfo the caller sees (psgpu_finish).
//
// Host only, and not embedded for hiprtc.  A plain C++ program (tests/cpp/plan_check.cpp,
// run_verdict_check.cpp) defines PSGPU_MODEL_NO_HIP first and needs no ROCm headers.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>

#include "../../include/parsip_gpu.h"
#include "psgpu_group_plan.h"
#include "psgpu_model.h"

namespace psgpu {

// The launch options of a context (psgpu_set_option and their environment overrides).
struct LaunchOptions {
    int vertexBlocksPerCU = 16;  // persistent k_vertex / k_finish grids (256-thread blocks)
    int finishBlocksPerCU = 8;
    int finishQuad = 2;  // PSGPU_OPT_FINISH_QUAD: 0 one lane, 1 a quad, 3 a pair of lanes per vertex, 2 by the last run's vertex count
    int vertexWide = 2;  // PSGPU_OPT_VERTEX_WIDE: 0 a quad, 1 one lane per vertex, 2 by the last run's vertex count
    int treeSplit = 0;   // PSGPU_OPT_TREE_SPLIT: 1 k_precheck / k_mpu walk the root's two subtrees in two waves
    int fusedSurface = 2;  // PSGPU_OPT_FUSED_SURFACE: k_vertex + k_finish in one launch (k_surface)
    int front = 2;         // PSGPU_OPT_FRONT: k_precheck + k_mpu in one launch (k_front)
    int sieve = 0;         // PSGPU_OPT_SIEVE: k_sieve ahead of S1: 0 never (default: measured slower, DESIGN.md §4
                           // "Round 12"), 1 whenever it applies, 2 unless the run is alone
    uint32_t splitMaxQueued = 1024;  // PSGPU_OPT_SPLIT_MAX_QUEUED: tree split 2 applies up to this many S2 MPUs
                                     // (psgpu_create: 4 per CU; C3's 1/8 shares queue ~800, 1/4 ~1,600)
    int gridFit = 1;       // k_vertex / k_finish grids sized from the last run's vertices, capped
                           // at the persistent grids (PSGPU_GRID_FIT=0: the persistent grids;
                           // C4 1/8 shares -5 %, full grids neutral: profiles/r05_grid_fit_ab2.txt)
    int mpuMarginDiv = 4;  // k_mpu grid: last run's queued MPUs + 1/this (re-run if short)
};

// What the last finished run of a context left for sizing the next one.
struct LastRun {
    bool haveQueued = false;  // lastQueued describes the current range and lattice
    uint32_t lastQueued = 0;  // S1 survivors queued for S2
    uint32_t lastSubMax = 0;  // the largest k_front sub-queue (0: that run took no k_front)
    uint32_t lastV = 0;       // vertices (0: none yet)
};

struct PlanInput {
    int numCUs;
    uint64_t bricks;    // 2x2x2 bricks of MPUs that cover the range (k_precheck's items)
    uint32_t mpuCount;  // > 0
    LaunchOptions opt;
    LastRun last;
    bool alone;       // enqueued while no other run of the process is pending on the device
    bool crowded;     // ... or while 4 or more other contexts have runs pending on it
    bool mpuTicks;    // the run records per-MPU ticks (MPUSTATS)
    bool splittable;  // the model's walk splits at the root
    // the loaded module: none (the interpreter), and which of the optional kernels it has
    bool jit, hasPrecheckS, hasSurface, hasSurfaceW, hasFront, hasFrontS;
    bool separate;   // finish re-runs a run whose in-kernel wait gave up: the separate kernels
    bool shortGrid;  // test hook (debug bit 20): a k_mpu grid that falls short (finish re-runs)
    bool sievable = false;  // culling is on and the model has a root-zero set (k_sieve can prove bricks dead)
};

struct LaunchPlan {
    bool split;        // the tree-split kernels (k_precheck_s / k_mpu_s, or k_front_s)
    bool front;        // k_precheck + k_mpu in one launch (k_front)
    bool surface;      // k_vertex + k_finish in one launch (k_surface)
    bool surfaceWide;  // ... its variant with one lane per vertex (k_surface_w)
    uint32_t vpwVertex;  // k_vertex layout, vertices per wave: 16 or 64
    uint32_t vpwFinish;  // k_finish layout: 16, 32 or 64
    uint32_t mpb;        // MPUs (bricks) per k_mpu (k_precheck) block: 2 with the split, else 4
    uint32_t preBlocks, mpuBlocks, fqCap, scanChunks, scanBlocks;  // Params' fields of these names
    uint32_t gridVertex, gridFinish;  // the separate kernels' grids (0 with k_surface)
    uint32_t gridSurface;             // k_surface's grid (0 without)
    uint32_t sieve;                   // 1: k_sieve runs ahead of S1, whose waves take its live list
};
static_assert(sizeof(LaunchPlan) == 4 + 12 * sizeof(uint32_t), "no padding: plans are compared with memcmp");

// k_front sub-queue capacity for a k_precheck grid of `blocks` blocks of `mpb` bricks: every
// 8th block's bricks x 8 MPUs
inline uint32_t front_sub_cap(uint32_t blocks, uint32_t mpb) { return 8u * mpb * ((blocks + 7u) / 8u); }
// ... for both k_precheck grids (2 and 4 bricks per block)
inline uint32_t front_cap(uint64_t bricks) {
    const uint32_t b = (uint32_t)bricks;
    return std::max(front_sub_cap((b + 1u) / 2u, 2u), front_sub_cap((b + 3u) / 4u, 4u));
}

// k_precheck covers the MPU range with 2x2x2 bricks of MPUs (one per wavefront: a
// compact box for its culling test), whole brick rows along x: the first brick row and the
// bricks along each axis (Params::brickI0, brickDims).
struct BrickLayout {
    uint32_t i0 = 0, dims[3] = {0, 0, 0};
};
inline BrickLayout brick_layout(const uint32_t dims[3], uint32_t mpuBegin, uint32_t mpuCount) {
    const uint32_t nyz = dims[1] * dims[2];
    const uint32_t first = nyz ? mpuBegin / nyz : 0;
    const uint32_t last = (nyz && mpuCount) ? (mpuBegin + mpuCount - 1) / nyz : first;
    BrickLayout b;
    b.i0 = first / 2;
    b.dims[0] = mpuCount ? last / 2 - first / 2 + 1 : 0;
    b.dims[1] = (dims[1] + 1) / 2;
    b.dims[2] = (dims[2] + 1) / 2;
    return b;
}
inline uint64_t brick_count(const BrickLayout& b) { return (uint64_t)b.dims[0] * b.dims[1] * b.dims[2]; }
// The brick permutation of k_precheck: stride 1 keeps the lattice order; otherwise a
// stride near n / golden ratio, coprime with n, so consecutive wave slots (one block, one
// CU) take bricks far apart and the bricks crossed by the surface spread over the chip.
inline uint32_t brick_stride(uint32_t n, bool spread) {
    if (!spread || n < 3) return 1u;
    for (uint32_t s = (uint32_t)(n * 0.6180339887) | 1u; s > 1; --s)
        if (std::gcd(s, n) == 1u) return s;
    return 1u;
}

inline LaunchPlan plan_launch(const PlanInput& in) {
    const LaunchOptions& o = in.opt;
    const LastRun& last = in.last;
    LaunchPlan pl{};  // every byte zero (no padding): graph replay compares plan bytes
    const uint64_t cus = (uint64_t)in.numCUs;

    // k_precheck / k_mpu with the walk split at the root (two waves per brick / MPU)
    // (2: when the last finished run of this range queued at most splitMaxQueued MPUs for S2 --
    // a launch too small to fill the device, whose span is its heaviest items' walks)
    pl.split = in.jit && in.hasPrecheckS && in.splittable &&
               (o.treeSplit == 1 || (o.treeSplit == 2 && last.haveQueued && last.lastQueued <= o.splitMaxQueued));
    pl.mpb = pl.split ? 2u : (uint32_t)kMpusPerBlock;
    pl.preBlocks = (uint32_t)((in.bricks + pl.mpb - 1) / pl.mpb);

    // k_precheck + k_mpu as one launch (k_front) for the next run: 1 forces it, 2 (default) when
    // the k_precheck grid is at most 8 blocks per CU -- C3 and its rank shares, whose step the
    // boundary and the S1 tail weigh on (the driver's C3 window -7 %, one engine -2.4 %), not C5's
    // 512^3 frame (13 k S1 blocks: +4.6 %, the fused kernel's registers cost its S1 waves a slot;
    // profiles/r06_front_ab.txt).  Never with per-MPU ticks (MPUSTATS: S1 and S2 would write an
    // MPU's tick words from two XCDs in one launch), on a crowded device, on the interpreter, or
    // while finish re-runs a run whose in-kernel wait gave up (separate).
    pl.front = in.jit && o.front != 0 && !in.separate && !in.crowded && !in.mpuTicks &&
               (pl.split ? in.hasFrontS : in.hasFront) &&
               (o.front == 1 || (in.bricks + pl.mpb - 1) / pl.mpb <= 8u * cus);

    // k_sieve ahead of S1 (no S1 wave for a brick no primitive reaches): where it can prove
    // anything (sievable), never with per-MPU ticks (a dead brick's MPUs have no S1 wave to time);
    // 2: not for a run alone on the device, whose span is its heaviest S1 waves and which
    // would only pay the extra kernel boundary.  The S1 grid keeps its size: the waves past the
    // list exit at once.
    pl.sieve = in.sievable && !in.mpuTicks && (o.sieve == 1 || (o.sieve == 2 && !in.alone)) ? 1u : 0u;

    pl.fqCap = front_sub_cap(pl.preBlocks, pl.mpb);
    if (pl.front) {
        // k_front's S2 blocks: 8 per row, a row takes mpb entries of each sub-queue; rows for the
        // last run's largest sub-queue + 1/4 (or every entry of a sub-queue without a last run)
        const uint32_t sub = !last.haveQueued ? pl.fqCap
                             : (last.lastSubMax ? last.lastSubMax : (last.lastQueued + 7u) / 8u) + last.lastQueued / 32u + 32u;
        const uint32_t rows = (std::min(sub, pl.fqCap) + pl.mpb - 1u) / pl.mpb;
        pl.mpuBlocks = 8u * std::max(1u, rows);
    } else {
        // k_mpu: one wave per queued survivor, as many as the last finished run queued + 1/4
        // (a run that queues more is re-run by finish(): the grid then fits exactly)
        const uint32_t maxBlocks = (in.mpuCount + pl.mpb - 1) / pl.mpb;
        const uint32_t margin = last.lastQueued / (uint32_t)o.mpuMarginDiv + (o.mpuMarginDiv > 4 ? 64u : 256u);
        const uint32_t want = last.haveQueued ? (last.lastQueued + margin + pl.mpb - 1) / pl.mpb : maxBlocks;
        pl.mpuBlocks = std::max(1u, std::min(maxBlocks, want));
    }
    if (in.shortGrid) pl.mpuBlocks = pl.front ? 8u : 1u;  // the test hook, applied last

    // the offsets scan: k_vertex's (k_surface's) first scanBlocks blocks, all co-resident
    pl.scanChunks = std::max(1u, (in.mpuCount + kScanItems * kScanMaxBlocks - 1) / (kScanItems * kScanMaxBlocks));
    pl.scanBlocks = (in.mpuCount + kScanItems * pl.scanChunks - 1) / (kScanItems * pl.scanChunks);

    // k_finish layout for the next run (vertices per wave): a quad of lanes per vertex (16) when
    // the last run's vertices, 16 per wave, fit the persistent grid's waves in one pass (each
    // wave then walks a quarter of what a 64-vertex wave does), else a pair of lanes (32) when
    // they do 32 per wave, otherwise one lane per vertex (64: fewest waves in total).
    // A run alone on its device takes at most 32 per wave: the spans, not the total work, set
    // its time (C3 full grid, one engine: 0.1077 vs 0.1110 ms with the quad k_vertex).
    // The interpreter takes these layouts too.
    const uint64_t wavesF = cus * (uint64_t)o.finishBlocksPerCU * 4u;
    pl.vpwFinish = o.finishQuad == 0 ? 64u
                   : o.finishQuad == 1 ? 16u
                   : o.finishQuad == 3 ? 32u
                   : last.lastV == 0 ? 64u
                   : last.lastV <= 16u * wavesF ? 16u
                   : (last.lastV <= 32u * wavesF || in.alone) ? 32u
                   : 64u;

    // k_vertex layout for the next run (vertices per wave): one lane per vertex (64: each lane's
    // 4 edge samples as one walk, the least total work) when the last run's vertices, 16 per
    // wave, would take more than one pass of the persistent grid; otherwise a quad of lanes per
    // vertex (16: a quarter of the walk per wave, shorter spans), as a lone run always does.
    // The interpreter has the quad layout only.
    const uint64_t wavesV = cus * (uint64_t)o.vertexBlocksPerCU * 4u;
    pl.vpwVertex = !in.jit || o.vertexWide == 0 ? 16u
                   : o.vertexWide == 1 ? 64u
                   : (last.lastV > 16u * wavesV && !in.alone) ? 64u
                   : 16u;

    // k_vertex + k_finish as one launch (k_surface) for the next run: 1 forces it, 2 (default) when
    // both would take their quad layouts (a launch too small to fill the device: its step is the
    // launch floor); only with the small-launch kernels (compiled with the split),
    // never on the interpreter, on a crowded device or in a separate re-run
    if (in.jit && in.hasSurface && o.fusedSurface != 0 && !in.separate && !in.crowded) {
        if (o.fusedSurface == 3) {  // the wide variant, every launch
            pl.surface = pl.surfaceWide = in.hasSurfaceW;
        } else {
            // a run alone on the device (a blocking caller, a frame-at-a-time editor) is bound by its
            // spans: the quad layouts in one launch, while their waves fill the device at most ~8 times
            // (C3 alone 0.110 vs 0.115 ms; C5's 512^3 frame, far more vertices, 0.613 vs 0.600:
            // profiles/r06_latency_ab.txt)
            const uint64_t loneMaxV = 16ull * 8ull * 24ull * cus;  // 16 a wave, 24 waves a CU, 8 passes
            pl.surface = o.fusedSurface == 1 ||
                         (last.lastV != 0 && ((in.alone && last.lastV <= loneMaxV) || (pl.vpwVertex == 16 && pl.vpwFinish == 16)));
        }
    }

    // The grids: persistent (blocks per CU), or with gridFit fitted to the last finished run: a
    // wave per batch of its vertices + 1/8 (the kernels stride over any rest), not the persistent
    // grids' mostly empty waves.  Whichever kernel runs the scan never has fewer than scanBlocks.
    const uint32_t persistV = (uint32_t)(in.numCUs * o.vertexBlocksPerCU);
    const uint32_t persistF = (uint32_t)(in.numCUs * o.finishBlocksPerCU);
    const bool fit = o.gridFit && last.lastV;
    const uint64_t vv = (uint64_t)last.lastV + last.lastV / 8 + 256;
    const auto fitted = [&](uint32_t grid, uint64_t perBlock) {
        return fit ? std::min<uint32_t>(grid, (uint32_t)((vv + perBlock - 1) / perBlock)) : grid;
    };
    if (pl.surface) {
        // both quad layouts in one launch: the vertex grid (16 per wave), or one lane per vertex:
        // k_finish's grid (64 per wave)
        const uint32_t persist = std::max(pl.surfaceWide ? persistF : persistV, pl.scanBlocks);
        pl.gridSurface = std::max(pl.scanBlocks, fitted(persist, pl.surfaceWide ? 256u : 64u));
    } else {
        pl.gridVertex = std::max(pl.scanBlocks, fitted(std::max(persistV, pl.scanBlocks), 4ull * pl.vpwVertex));
        pl.gridFinish = fitted(persistF, 4ull * pl.vpwFinish);
    }
    return pl;
}

// ---------------------------------------------------------------------------
// The verdict on a finished run.

// A finished run's counters over its shards: sums, and the largest shard's vertices and triangles.
struct ShardSums {
    uint32_t v = 0, t = 0, s = 0, p = 0, b = 0, maxV = 0, maxT = 0;
    explicit ShardSums(const DevCounters& h) {
        for (int k = 0; k < kShards; ++k) {
            v += h.shard[k].v;
            t += h.shard[k].t;
            s += h.shard[k].s;
            p += h.shard[k].p;
            b += h.shard[k].b;
            maxV = std::max(maxV, h.shard[k].v);
            maxT = std::max(maxT, h.shard[k].t);
        }
    }
};

// What a run may write: the compact mesh's vertices and triangles, and each shard's vertex and
// triangle records.  Also what a run did write (RunVerdict::used) and the most any run has.
struct Caps {
    uint32_t v, t, shardV, shardT;
};
inline bool within(const Caps& a, const Caps& cap) {
    return a.v <= cap.v && a.t <= cap.t && a.shardV <= cap.shardV && a.shardT <= cap.shardT;
}
inline Caps caps_max(const Caps& a, const Caps& b) {
    return {std::max(a.v, b.v), std::max(a.t, b.t), std::max(a.shardV, b.shardV), std::max(a.shardT, b.shardT)};
}

inline uint32_t protocol_error(const DevCounters& h) { return h.error | h.surfaceErr; }

struct RunVerdict {
    Caps used;           // what the run appended (the device counts past a full buffer, writing nothing)
    LastRun last;        // what it leaves for sizing the next run
    bool gridShort;      // S1 queued more than the run's S2 blocks take
    bool fits;           // the grid and the four capacities held: the output is whole
    uint32_t protocol;   // an in-kernel wait gave up (DevCounters::error | surfaceErr); 0 for an empty range
};

// `h`: the counters k_finish published, `run`: the plan the run was launched with.  An empty range
// launches nothing: its grid is never short and it has no protocol error, but the counters (the
// host zeroes them for such a run) are still held against the capacities.
inline RunVerdict judge_run(const DevCounters& h, const LaunchPlan& run, uint32_t mpuCount, const Caps& caps) {
    const ShardSums sum(h);
    RunVerdict r{};
    r.used = {sum.v, sum.t, sum.maxV, sum.maxT};
    r.gridShort = mpuCount > 0 && sum.p > run.mpb * run.mpuBlocks;
    if (run.front) {  // k_front: each sub-queue against its own rows of S2 blocks
        uint32_t sub = 0;
        for (int k = 0; k < 8; ++k) sub = std::max(sub, h.shard[k].p);
        r.gridShort = mpuCount > 0 && sub > run.mpb * (run.mpuBlocks / 8u);
        r.last.lastSubMax = sub;
    }
    r.last.lastQueued = sum.p;
    r.last.lastV = sum.v;
    r.last.haveQueued = mpuCount > 0;
    r.fits = !r.gridShort && within(r.used, caps);
    r.protocol = mpuCount ? protocol_error(h) : 0u;
    return r;
}

// The capacities to re-run a run that did not fit with: what it used and a margin, never less than before.
inline Caps grown(const Caps& caps, const RunVerdict& r) {
    const Caps& u = r.used;
    return caps_max(caps, {u.v + u.v / 8 + 1024, u.t + u.t / 8 + 1024, u.shardV + u.shardV / 4 + 256, u.shardT + u.shardT / 4 + 256});
}
// The capacities of the next run from the most any finished run used: + 1/4, never less than before.
inline Caps grown_ahead(const Caps& caps, const Caps& seen) {
    return caps_max(caps, {seen.v + seen.v / 4, seen.t + seen.t / 4, seen.shardV + seen.shardV / 4, seen.shardT + seen.shardT / 4});
}

// What psgpu_finish reports of a collected run.  reran: finish launched it more than once.
inline PsMeshInfo mesh_info(const DevCounters& h, const LaunchPlan& run, uint32_t mpuCount, bool reran) {
    const ShardSums sum(h);
    PsMeshInfo I;
    memset(&I, 0, sizeof(I));
    I.ctMPUs = mpuCount;
    I.ctPassedPrecheck = mpuCount ? sum.p + sum.b : 0;
    I.ctSurfaceMPUs = mpuCount ? sum.s : 0;
    I.ctVertices = mpuCount ? sum.v : 0;
    I.ctTriangles = mpuCount ? sum.t : 0;
    I.firstOverflowMPU = (mpuCount && h.firstOverflow != 0x7fffffff) ? h.firstOverflow : -1;
    I.ctFieldMPUs = mpuCount ? sum.p : 0;
    I.ctLaneEvals = lane_evals(mpuCount, I.ctFieldMPUs, I.ctVertices);
    I.launchFlags = mpuCount == 0 ? 0u
                    : (run.split ? PSGPU_LAUNCH_TREE_SPLIT : 0u) | (run.surface ? PSGPU_LAUNCH_SURFACE : 0u) |
                          (run.front ? PSGPU_LAUNCH_FRONT : 0u) | (reran ? PSGPU_LAUNCH_RERUN : 0u) |
                          (run.sieve ? PSGPU_LAUNCH_SIEVE : 0u);
    return I;
}

}  // namespace psgpu
